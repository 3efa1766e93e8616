// attention_args.h — kernel-argument block shared by attention.hip (VALU row-owner kernels, any
// head dims <= 64) and attention_mfma.hip (matrix-core kernels for d_k = d_v = 4).
#pragma once
#include "common.h"

struct PgAttnArgs {
  const float* q; const float* k; const float* v; const float* o; const float* d_o;
  const float* lse2_in;
  float* o_out; float* lse2_out; float* delta; float* dq; float* dk; float* dv;
  int N, heads, L, dk_dim, dv_dim, strict;
  long q_bs, k_bs, v_bs, o_bs, do_bs, dq_bs, dk_bs, dv_bs;
  float scale, scale2;  // 1/sqrt(dk), log2(e)/sqrt(dk)
  int blocks_per_wg;    // 64-row blocks per workgroup (<= 16); waves = ceil(blocks_per_wg / 2)
  int kt, kt2;          // VALU kernels: rows per LDS tile (fwd/dQ resp. dK/dV), multiples of 64,
                        // sized so that a whole (n, head) fits when LDS allows: barriers between
                        // tiles would re-serialise the balanced pairing
  int lp, vec;          // MFMA kernels: LDS plane stride (== 16 mod 64); float4 staging allowed
  // MFMA kernels: the 64-row blocks each wave of the workgroup processes, heaviest first (LPT
  // assignment made on the host so that every wave — and with a wave count that is a multiple of 4,
  // every SIMD — gets the same share of the causal triangle)
  unsigned char bcount[8];
  unsigned char blist[8][16];
  // MFMA query-owner kernels (forward, dQ): when the 16-query groups do not fill whole 64-query blocks, the
  // short block is block 0 and every later block starts qshift = 64 - 16 * (groups of block 0) queries early
  // (0: whole blocks). Wave-uniform; pg_attn_query_block() is the only place that reads it.
  int qshift;
};

// Queries [q0, q0 + 16 * ngrp) of block blk of the forward / dQ kernels (device and host planner alike).
struct PgAttnQueryBlock { int q0, ngrp; };
__host__ __device__ inline PgAttnQueryBlock pg_attn_query_block(int blk, int qshift) {
  PgAttnQueryBlock b;
  b.q0 = blk == 0 ? 0 : 64 * blk - qshift;
  b.ngrp = blk == 0 ? 4 - (qshift >> 4) : 4;
  return b;
}

enum { PG_ATTN_FWD = 0, PG_ATTN_DQ = 1, PG_ATTN_DKV = 2, PG_ATTN_BWD = 3 /* fused dQ + dK + dV (d_k = d_v = 4) */ };

// Where a launch goes and how it is laid out: decided ONCE, by attn_route (attention.hip), which asks pg_attn_mfma_route
// (and through it pg_attn_k4_route) in the launch's order and falls back to the VALU kernels. The launchers below and the
// host-only query pg_attn_route read this struct; none of them decides anything again.
struct PgAttnRoute {
  int family;            // PG_ATTN_FAM_*
  int fused_on;          // the fused-backward switch as found
  int DK, DV, QB;        // template instantiation: VALU Cfg<DK, DV>; k4 <DKT, DVT, QB>; d = 4: 4, 4, 0
  int grid[3], block, lds;
  int bpw, kt, kt2;      // VALU: 64-row blocks per workgroup, rows per LDS tile (fwd / dQ resp. dK/dV)
  int waves, lp, vec;    // waves per workgroup; d = 4: plane stride, float4 stores
  int variant;           // d = 4: dK/dV 1 = bf16x3 score tile; fused backward: compile-time plane stride (848 / 1040 / 0)
  const void* plan;      // d = 4: the AttnPlan of (which, L, waves)
};

// What a launch reads from its pointers and strides, as PG_ATTN_R_* flags.
inline int pg_attn_route_flags(const PgAttnArgs& a) {
  auto mis = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
  int f = 0;
  if (mis(a.q) || mis(a.k) || mis(a.v)) f |= PG_ATTN_R_QKV_MISALIGNED;
  if (mis(a.o_out)) f |= PG_ATTN_R_O_MISALIGNED;
  if (mis(a.d_o) || mis(a.lse2_in) || mis(a.delta)) f |= PG_ATTN_R_GRADIN_MISALIGNED;
  if (mis(a.dq)) f |= PG_ATTN_R_DQ_MISALIGNED;
  if (mis(a.dk) || mis(a.dv)) f |= PG_ATTN_R_DKV_MISALIGNED;
  if ((a.q_bs | a.k_bs | a.v_bs) % 4 != 0) f |= PG_ATTN_R_QKV_STRIDE;
  if (a.o_bs % 4 != 0) f |= PG_ATTN_R_O_STRIDE;
  if (a.do_bs % 4 != 0) f |= PG_ATTN_R_DO_STRIDE;
  if (a.dq_bs % 4 != 0) f |= PG_ATTN_R_DQ_STRIDE;
  if ((a.dk_bs | a.dv_bs) % 4 != 0) f |= PG_ATTN_R_DKV_STRIDE;
  return f;
}

// attention_mfma.hip / attention_k4.hip. *_route: 1 and r filled in if the family takes (which, shape, flags), 0 and r untouched
// if not (pg_attn_mfma_route passes everything but d_k = d_v = 4 on to pg_attn_k4_route). *_launch: launches what r says;
// launch errors are left for PG_LAUNCH_CHECK.
int pg_attn_mfma_route(int which, int N, int heads, int L, int dk, int dv, int flags, PgAttnRoute& r);
int pg_attn_k4_route(int which, int N, int heads, int L, int dk, int dv, int flags, PgAttnRoute& r);
void pg_attn_mfma_launch(int which, const PgAttnArgs& a, const PgAttnRoute& r, hipStream_t st);
void pg_attn_k4_launch(int which, const PgAttnArgs& a, const PgAttnRoute& r, hipStream_t st);
