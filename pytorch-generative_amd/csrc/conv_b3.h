// conv_b3.h — what conv_b3.hip (the bf16x3 convolution, format PG_CONV_FMT_B3) offers to conv_mfma.hip's exported entry points.
#pragma once
#include "common.h"

// the format takes the problem (K channels, M channels, taps, output size, row / column extent of the tap list)
int pg_b3_applicable(int Kc, int M, int T, int OH, int OW, int hr, int hc);
size_t pg_b3_frag_floats(int Kc, int M, int T);
// either destination may be null (then only the other orientation is packed)
int pg_b3_pack2(const float* w, float* wfrag_fwd, float* wfrag_dgrad, int Cout, int Cin, int KH, int KW,
                int T, const int* tap_u, const int* tap_v, hipStream_t st, int gate_order = 0);
// gate != 0 (1 + PG_GATE_*; round 6): the launch must be the wide kernel (Cout % 128 == 0, at most one dense residual) — it then also writes
// gate_out = gate_res + act(a) * sigmoid(b) for [a | b] = out (+ res); pg_b3_gate_fusable() says beforehand whether a shape qualifies.
// dual_out2 != null: the "dual" 1x1 data gradient (pg_conv2d_mfma_dual); pg_b3_dual_ok() says whether a shape qualifies.
int pg_b3_conv(const float* in, const float* wfrag, const float* bias, const float* res, float* out,
               int N, int Cin, int IH, int IW, int Cout, int OH, int OW, int T, const int* tap_dr,
               const int* tap_dc, int in_act, const float* dact_src, int dact, int out_act,
               const float* res2, long res_bs, long res2_bs, hipStream_t st, int gate = 0, const float* gate_res = nullptr,
               float* gate_out = nullptr, float* dual_out2 = nullptr);
int pg_b3_dual_ok(int Cin, int Cout, int OH, int OW);
int pg_b3_gate_fusable(int Cin, int Cout, int T, int OH, int OW, const int* tap_dr, const int* tap_dc);
