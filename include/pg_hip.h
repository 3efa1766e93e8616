/*
 * pg_hip.h — C-ABI of libpg_hip.so: the MI355X (gfx950) kernels behind the
 * pytorch_generative.nn operator surface (masked conv + causal attention hot path).
 *
 * The reference (EugenHotaj/pytorch-generative) has no FFI: its arithmetic is torch
 * (SURVEY.md §8b). Each entry point below therefore cites the reference *call site*
 * whose torch op it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *  - plain pointers + sizes; all tensors fp32, dense NCHW ("L" = H*W contiguous).
 *  - every pointer is a DEVICE pointer owned by the caller (PyTorch's allocator);
 *    the library never allocates, frees, retains, or synchronises (hipGraph-capturable).
 *  - `stream` is a hipStream_t passed as void*.
 *  - return 0 on success; <0 = argument error (PG_E*); >0 = hipError_t of the launch.
 *    pg_last_error() returns a thread-local message for the last non-zero return.
 *  - functions are re-entrant (called from the autograd thread as well as the main thread).
 */
#ifndef PG_HIP_H_
#define PG_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PG_ABI_VERSION 3

#define PG_EINVAL (-1)  /* bad argument */
#define PG_ESHAPE (-2)  /* shape outside what the kernels support (no silent fallback) */

#define PG_MAX_TAPS 64

/* activation ids (pg_act_*, conv prologues) */
#define PG_ACT_NONE 0
#define PG_ACT_RELU 1 /* nn.ReLU: models/autoregressive/pixel_cnn.py:33-50 */
#define PG_ACT_ELU 2  /* F.elu alpha=1: models/autoregressive/pixel_snail.py:27-28 */
#define PG_ACT_GELU 3 /* nn.GELU() exact erf: models/autoregressive/image_gpt.py:44 */
/* only as the `dact` of pg_conv2d_mfma: dact_src holds ELU's OUTPUT y, derivative = y > 0 ? 1 : y + 1
 * (a producer convolution fused F.elu into its epilogue, pixel_snail.py:54) */
#define PG_ACT_ELU_OUT 4

/* gate kinds for pg_gated_* (nn/convolution.py:46-66) */
#define PG_GATE_TANH 0     /* tanh(a)*sigmoid(b): gated_pixel_cnn.py:57 */
#define PG_GATE_IDENTITY 1 /* a*sigmoid(b): pixel_snail.py:50 */

int pg_abi_version(void);
const char* pg_last_error(void);

/* ---------------------------------------------------------------------------------------
 * Direct 2-D convolution over an explicit tap list (stride 1).
 * Replaces torch.nn.Conv2d.forward as reached from
 *   CausalConv2d.forward           nn/convolution.py:41-43  (taps = the mask's non-zero taps)
 *   every nn.Conv2d on the path    gated_pixel_cnn.py:63-96, pixel_snail.py:41-55 (pad+crop
 *                                  become tap offsets + the out extent), attention.py:105-118,
 *                                  image_gpt.py:40-48 (1x1)
 * out[n,co,r,c] = bias[co] + sum_ci sum_t wpk[ci][t][co] * act(in[n,ci,r+dr[t],c+dc[t]])
 * (zero outside the input extent). `wpk` is the packed weight made by pg_pack_conv_weight.
 * The same kernel is the data-gradient: call it with the transposed pack and negated taps.
 * `res` (optional, may be NULL) is added to the result (fused residual).
 * `dact_src`/`dact` (optional): the result is multiplied by act'(dact_src) — the data gradient of
 * a convolution whose forward fused `in_act` (dact_src = that convolution's raw input); behind `res` if both are
 * given. A 1x1 problem (one tap at offset 0, IH x IW == OH x OW) takes a derivative source only with
 * in_act == PG_ACT_NONE (PG_EINVAL otherwise: a data gradient has no input activation).
 * ------------------------------------------------------------------------------------- */
int pg_conv2d_taps(const float* in, const float* wpk, const float* bias, const float* res,
                   float* out, int N, int Cin, int IH, int IW, int Cout, int OH, int OW,
                   int T, const int* tap_dr, const int* tap_dc, int in_act,
                   const float* dact_src, int dact, void* stream);

/* packed-weight helper: wpk[a][t][b] (b padded to b_pad, zero filled),
 *   transpose==0: = w[b][a][tap_u[t]][tap_v[t]]   (forward:   a=Cin,  b=Cout)
 *   transpose==1: = w[a][b][tap_u[t]][tap_v[t]]   (data grad: a=Cout, b=Cin)
 * w is the torch layout (Cout, Cin, KH, KW) (nn/convolution.py:35-36). */
int pg_pack_conv_weight(const float* w, float* wpk, int Cout, int Cin, int KH, int KW, int T,
                        const int* tap_u, const int* tap_v, int transpose, int b_pad,
                        void* stream);
/* number of floats pg_pack_conv_weight writes */
size_t pg_packed_weight_floats(int a, int T, int b);
/* padded extent of b the conv kernel expects */
int pg_conv_b_pad(int b);

/* ---------------------------------------------------------------------------------------
 * The same convolution as an implicit GEMM on the fp32 matrix cores (csrc/conv_mfma.hip):
 * M = output channels, N = output pixels, K = (input-channel group of 4, tap). Replaces the same
 * reference call sites as pg_conv2d_taps (nn/convolution.py:41-43, gated_pixel_cnn.py:63-96,
 * pixel_snail.py:41-55, every 1x1 convolution) once both channel counts fill MFMA tiles
 * (pg_conv_mfma_supported != 0; otherwise call pg_conv2d_taps). `wfrag` = A fragments made by
 * pg_pack_conv_weight_frag (transpose = 1 + negated taps: the data gradient).
 * Epilogue order: + bias, out_act (PG_ACT_*), + res, * dact'(dact_src).
 * ------------------------------------------------------------------------------------- */
int pg_conv2d_mfma(const float* in, const float* wfrag, const float* bias, const float* res,
                   float* out, int N, int Cin, int IH, int IW, int Cout, int OH, int OW, int T,
                   const int* tap_dr, const int* tap_dc, int in_act, const float* dact_src,
                   int dact, int out_act, int fmt, void* stream);
/* The same with the full epilogue of the bf16x3 format:
 *   out = out_act(conv + bias) * act'(dact_src) + res + res2
 * (the derivative BEFORE the residuals). In a data gradient res / res2 are the pass-through gradients
 * of skip connections on the convolution's input (autograd's gradient-sum `add` kernels, fused);
 * res_bs / res2_bs: their batch strides in floats (0 = dense Cout * OH * OW), so that a residual may
 * be a channel slice of a wider tensor (the slice of a concatenation's gradient). fmt = PG_CONV_FMT_F32
 * accepts only res2 = NULL, dense res and not (res and dact_src) together. */
int pg_conv2d_mfma_ex(const float* in, const float* wfrag, const float* bias, const float* res,
                      float* out, int N, int Cin, int IH, int IW, int Cout, int OH, int OW, int T,
                      const int* tap_dr, const int* tap_dc, int in_act, const float* dact_src,
                      int dact, int out_act, int fmt, const float* res2, long res_bs, long res2_bs,
                      void* stream);
/* Round 6: the convolution of a gated block together with its GatedActivation (+ residual) — nn/convolution.py:62-66 behind the
 * 2C-channel convolution of pixel_snail.py:41-56 and gated_pixel_cnn.py:63-96: out (N, 2C, OH, OW) = conv(in_act(in)) + bias + res is
 * written as usual (the gate's backward, pg_gated_bwd, reads it; res = the convolution's own residual — GatedPixelCNN's link and
 * vertical-stack sums — or NULL) and gate_out (N, C, OH, OW) = gate_res + act(out[:, :C]) * sigmoid(out[:, C:]); gate_res may be
 * NULL. 2C must be a multiple of 128 on the bf16x3 format's wide kernel; pg_conv_gate_fusable() returns 1 for the shapes it takes.
 * wfrag: pg_pack_conv_weight_frag(fmt = PG_CONV_FMT_B3_GATE). */
int pg_conv_gate_fusable(int Cin, int Cout, int OH, int OW, int T, const int* tap_dr, const int* tap_dc);
int pg_conv2d_mfma_gate(const float* in, const float* wfrag, const float* bias, const float* res, float* out, int N, int Cin,
                        int IH, int IW, int Cout, int OH, int OW, int T, const int* tap_dr, const int* tap_dc, int in_act, int gate,
                        const float* gate_res, float* gate_out, void* stream);
/* Round 6: the "dual" 1x1 data gradient of PixelSNAIL's block tail (pixel_snail.py:109-119: both = elu(conv_a(..)) + r,
 * out = elu(conv_o(elu(both))) + x). conv_o's data gradient owes BOTH producers of its input their ELU derivatives (they were
 * called with the out_pre_scaled protocol). in = dy of conv_o (N, Cin, OH, OW), wfrag = pg_pack_conv_weight_frag(transpose = 1,
 * PG_CONV_FMT_B3), dact_src = both, r (N, Cout, OH, OW):
 *   d    = conv1x1(in) * act'(dact_src)                      (dact: PG_ACT_ELU for conv_o's own input activation)
 *   out  = d * elu'(a)  with elu(a) = dact_src - r           (gradient of conv_a's pre-activation)
 *   out2 = d * elu'(r's pre-activation)                      (gradient of r's producer's pre-activation)
 * both derivatives from the stored ELU outputs (y > 0 ? 1 : y + 1). Replaces two pg_act_bwd_from_out launches.
 * pg_conv_dual_ok() returns 1 for the shapes the bf16x3 1x1 kernel takes (<= 64 input channels of the forward convolution). */
int pg_conv_dual_ok(int Cin, int Cout, int OH, int OW);
int pg_conv2d_mfma_dual(const float* in, const float* wfrag, float* out, float* out2, int N, int Cin, int OH, int OW, int Cout,
                        const float* dact_src, int dact, const float* r, void* stream);
/* Two arithmetic back ends share this entry point; they differ in the weight-fragment FORMAT:
 *   PG_CONV_FMT_F32: v_mfma_f32_16x16x4_f32 on fp32 fragments (csrc/conv_mfma.hip);
 *   PG_CONV_FMT_B3:  every fp32 product as six v_mfma_f32_16x16x32_bf16 on exact three-way bf16
 *                    splits of both operands (csrc/conv_b3.hip; fp32-level accuracy, ~2.5x the rate).
 * pg_conv_mfma_supported returns the format to use for a (Cin -> Cout, T taps, OH x OW outputs,
 * input rows of IW, tap-list extent hr x hc) problem, or 0 (call pg_conv2d_taps instead). */
#define PG_CONV_FMT_F32 1
#define PG_CONV_FMT_B3 2
/* pack-only (forward orientation, Cout % 128 == 0): PG_CONV_FMT_B3 fragments with the output channels ordered so that each 64-channel
 * chunk holds 32 gate channels' two halves — tile m of chunk c = channels (Cout / 2) (m >> 1) + 32 c + 16 (m & 1) + 0..15. The format
 * pg_conv2d_mfma_gate reads (one wave then owns both operands of its gate channels); `out` is still written in natural order. */
#define PG_CONV_FMT_B3_GATE 3
int pg_conv_mfma_supported(int Cin, int Cout, int T, int OH, int OW, int IW, int hr, int hc);
/* Host only (no device call): which bf16x3 kernel instantiation a PG_CONV_FMT_B3 launch of this problem takes and how it is laid out —
 * the answer of the one route function the launch itself, pg_conv_dual_ok and pg_conv_gate_fusable read (csrc/conv_b3.hip: b3_route).
 * flags: PG_B3R_* (which optional operands the launch has); gate: 0 or 1 + PG_GATE_*. Fills out[0 .. PG_B3_ROUTE_INTS): kernel id (0 staged,
 * 1 1x1, 2 pipelined, 3 overlapped), GELU instantiation, MT, NT, CG, MS, GT, waves, staging slots per thread, two tiles per workgroup,
 * grid x, grid y, block size, LDS bytes, then TR, tile_h, tile_w, plane16, tiles_per_img, CIB, cgs, groups, ksteps, wslab4, xslots,
 * dump16, w_off16, ep_off, b_off, res_scale, "same residual twice" folded, min_dr, min_dc, g_tapoff[20], g_cg[20]. Returns 0, or the
 * status the launch would return (PG_ESHAPE) with the same message; PG_EINVAL for a null pointer, a short array or a bad dimension. */
#define PG_B3R_RES 1            /* res given */
#define PG_B3R_RES2 2           /* res2 given */
#define PG_B3R_RES2_SAME 4      /* ... and it is the same tensor as res */
#define PG_B3R_RES_STRIDED 8    /* res is a channel slice of a wider tensor */
#define PG_B3R_DACT_SRC 16      /* a derivative source is given */
#define PG_B3R_DUAL 32          /* pg_conv2d_mfma_dual's second output */
#define PG_B3R_IN_MISALIGNED 64 /* `in` is not 8-byte aligned */
#define PG_B3_ROUTE_INTS 73
int pg_conv_b3_route(int N, int Cin, int IH, int IW, int Cout, int OH, int OW, int T, const int* tap_dr, const int* tap_dc,
                     int in_act, int dact, int out_act, int gate, int flags, int* out, int out_len);
/* floats pg_pack_conv_weight_frag writes for K_channels contracted into M_channels over T taps */
size_t pg_conv_frag_floats(int K_channels, int M_channels, int T, int fmt);
/* wfrag[chunk][g*T + t][m][lane] = Wsel[64 chunk + 16 m + (lane & 15)][4 g + (lane >> 4)][t], with
 *   transpose==0: Wsel[o][c][t] = w[o][c][tap_u[t]][tap_v[t]]  (M = Cout, K channels = Cin)
 *   transpose==1: Wsel[o][c][t] = w[c][o][tap_u[t]][tap_v[t]]  (M = Cin,  K channels = Cout)
 * zero filled outside; w is the torch layout (Cout, Cin, KH, KW). */
int pg_pack_conv_weight_frag(const float* w, float* wfrag, int Cout, int Cin, int KH, int KW,
                             int T, const int* tap_u, const int* tap_v, int transpose, int fmt,
                             void* stream);
/* both orientations of one weight in ONE launch (either output may be NULL): the forward pass packs
 * the data-gradient fragments it will need in backward at the same time */
int pg_pack_conv_weight_frag2(const float* w, float* wfrag_fwd, float* wfrag_dgrad, int Cout,
                              int Cin, int KH, int KW, int T, const int* tap_u, const int* tap_v,
                              int fmt_fwd, int fmt_dgrad, void* stream);

/* Weight + bias gradient (MFMA f32 16x16x4). The result is ADDED to dw/db (the caller zeroes
 * them once per step); per-workgroup partial sums go through `workspace` and a second,
 * deterministic reduction kernel (no atomics). Replaces aten::convolution_backward's weight/bias
 * outputs.
 * dw[co][ci][tap_u[t]][tap_v[t]] += sum_{n,r,c} dy[n,co,r,c] * act(x[n,ci,r+dr[t],c+dc[t]])
 * db[co] += sum dy  (db may be NULL).
 * NOTE the reference's weight.grad is non-zero at masked taps (mask is applied to
 * weight.data outside autograd, nn/convolution.py:42) — pass all KH*KW taps for exact parity. */
int pg_conv2d_wgrad(const float* x, const float* dy, float* dw, float* db, int N, int Cin,
                    int IH, int IW, int Cout, int OH, int OW, int KH, int KW, int T,
                    const int* tap_dr, const int* tap_dc, const int* tap_u, const int* tap_v,
                    int in_act, float* workspace, size_t workspace_floats, void* stream);
/* floats of scratch pg_conv2d_wgrad needs for a (Cout, Cin, T) problem */
size_t pg_conv2d_wgrad_workspace_floats(int Cout, int Cin, int T);
/* Host only (no device call): which kernel a pg_conv2d_wgrad call of this problem launches and how it is laid out — the answer of the
 * one route function the launch itself reads (csrc/conv_wgrad.hip: wgrad_route). flags: PG_WGR_* (db given; x / dy not 16-byte
 * aligned). Fills out[0 .. PG_WGR_ROUTE_INTS):
 *   [0]     family: 0 x-copy bf16x3 (conv_wgrad_b3_kernel), 1 row ring (conv_wgrad_b3r_kernel), 2 shifted dy (conv_wgrad_b3s_kernel),
 *           3 fp32 1x1 (conv_wgrad_pw_kernel), 4 input layer (conv_wgrad_small_kernel), 5 generic fp32 (conv_wgrad_kernel)
 *   [1..4]  that family's template integers: x-copy T, MR, waves, CIT | ring T, WM, WN | shifted dy NR, NC | 1x1 NCOT, NCIT, ACT |
 *           input layer none | generic NT (taps per pass), NC, prefetch; unused ones 0
 *   [5..9]  grid x, y, z, block size, dynamic LDS bytes
 *   [10]    G, the partial rows the kernel writes and the reduction reads (= grid x)
 *   [11..13] TR (rows per tile; ring 1), tiles per image, total tiles (ring: (image, segment) units; 1x1: 16-pixel groups)
 *   [14..16] nseg, seg_rows (ring: row segments per image, rows per segment), PBR (bf16x3: 8-pixel blocks per row)
 *   [17..18] vec_dy, vec_x (float4 staging of dy / x)
 *   [19]    grid of wgrad_reduce_kernel (64 slots per workgroup)
 *   [20..22] row halo of the tap list, copies (x copies of x-copy / ring, dy copies of shifted dy), tap passes (generic)
 *   [23]    partial rows the workspace of pg_conv2d_wgrad_workspace_floats holds
 * The ablation / experiment switches (PG_AB_*, read by the variant libraries only) are honoured: the route is what THIS process would
 * launch. Returns 0, or the status the launch would return (PG_ESHAPE) with the same message; PG_EINVAL for a null pointer, a short
 * array or a bad dimension. */
#define PG_WGR_HAS_BIAS 1
#define PG_WGR_X_MISALIGNED 2
#define PG_WGR_DY_MISALIGNED 4
#define PG_WGR_ROUTE_INTS 24
int pg_conv2d_wgrad_route(int N, int Cin, int IH, int IW, int Cout, int OH, int OW, int KH, int KW, int T, const int* tap_dr,
                          const int* tap_dc, int in_act, int flags, int* out, int n_out);

/* w *= mask in place: nn/convolution.py:42 `self.weight.data *= self.mask`. */
int pg_mul_inplace(float* w, const float* mask, size_t n, void* stream);

/* ---------------------------------------------------------------------------------------
 * NCHW LayerNorm over C.  nn/convolution.py:69-75 (permute -> nn.LayerNorm(C) -> permute).
 * eps as given (1e-5), biased variance, affine. mean/rstd: (N*L) each, saved for backward.
 * ------------------------------------------------------------------------------------- */
int pg_nchw_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y,
                          float* mean, float* rstd, int N, int C, int L, float eps,
                          void* stream);
/* dgamma/dbeta are ADDED to (per-block partial rows through `workspace`, then a deterministic
 * reduce kernel; no atomics). */
int pg_nchw_layernorm_bwd(const float* x, const float* gamma, const float* mean,
                          const float* rstd, const float* dy, float* dx, float* dgamma,
                          float* dbeta, int N, int C, int L, float* workspace,
                          size_t workspace_floats, void* stream);
size_t pg_nchw_layernorm_bwd_workspace_floats(int N, int C, int L);
/* Same, with dx = LN backward + dx_add: the gradient of the residual (skip) branch that leaves the
 * same x — `x + f(LN(x))` in every transformer / PixelSNAIL block (image_gpt.py:50-52) — is added in
 * the kernel's epilogue instead of by a separate autograd accumulation pass. dx_add must not alias dx. */
int pg_nchw_layernorm_bwd_res(const float* x, const float* gamma, const float* mean,
                              const float* rstd, const float* dy, const float* dx_add, float* dx,
                              float* dgamma, float* dbeta, int N, int C, int L, float* workspace,
                              size_t workspace_floats, void* stream);

/* ---------------------------------------------------------------------------------------
 * Fused causal attention core.  nn/attention.py:147-160:
 *   S = q k^T / sqrt(dk); masked_fill(mask==0,-inf); softmax; masked_fill(mask==0, 0); @ v
 * with mask = tril(ones(L,L), -strict) (nn/attention.py:60-63), never materialised.
 * q,k: (N, heads*dk, L) channel-major; v,o: (N, heads*dv, L); head h owns channels
 * [h*d,(h+1)*d) (attention.py:134). *_bs = batch stride in floats (k and v are views into
 * the _kv conv output, attention.py:144). lse2: (N, heads, L) log2-domain logsumexp saved for
 * backward. A row with no allowed key (l=0, strict) yields zeros (attention.py:153-157).
 * Instantiated head dims (PG_ESHAPE otherwise): dk = dv = 4 and every (dk <= 4, dv <= 32) / (dk <= 16, dv <= 16) at
 * any L; dk in {4, 16, 32, 64} x dv in {16, 32, 64} for L % 16 == 0 with 16-byte aligned planes. The reference's
 * CausalAttention accepts any embed / head split: the Python host (ops.causal_attention) zero-pads other head dims
 * and sequence lengths to the next instantiated size — exact, see its docstring.
 * pg_causal_attn_bwd: dk = 4 with dv in {4, 16, 32} runs ONE fused kernel whose dq is summed with fp32 atomics
 * (run-to-run last-bit differences) while that kernel takes the shape: dv = 4 up to L = 1792 (its LDS planes), dv = 16 / 32 for
 * L % 16 == 0 with 16-byte aligned planes; otherwise, and after pg_attn_fused_bwd(0), the bit-reproducible two-kernel backward
 * runs. pg_attn_route tells which.
 * ------------------------------------------------------------------------------------- */
int pg_causal_attn_fwd(const float* q, const float* k, const float* v, float* o, float* lse2,
                       int N, int heads, int L, int dk, int dv, long q_bs, long k_bs, long v_bs,
                       long o_bs, int strict, void* stream);
/* dq/dk/dv written (not accumulated). delta: (N, heads, L) workspace. For d_k = d_v = 4 up to L = 1792 this
 * is ONE fused launch (attention_mfma.hip attn_bwd_m44_kernel: S, dP and exp2 evaluated once per pair; delta
 * is then not written); otherwise the two launches below. */
int pg_causal_attn_bwd(const float* q, const float* k, const float* v, const float* o,
                       const float* d_o, const float* lse2, float* delta, float* dq, float* dk,
                       float* dv, int N, int heads, int L, int dk_dim, int dv_dim, long q_bs,
                       long k_bs, long v_bs, long o_bs, long do_bs, long dq_bs, long dk_bs,
                       long dv_bs, int strict, void* stream);

/* The two launches of pg_causal_attn_bwd individually (same argument list): _dq writes dq and
 * delta, _dkv reads delta and writes dk, dv. Used by bench.py to time the dominant kernel. */
int pg_causal_attn_bwd_dq(const float* q, const float* k, const float* v, const float* o,
                          const float* d_o, const float* lse2, float* delta, float* dq, float* dk,
                          float* dv, int N, int heads, int L, int dk_dim, int dv_dim, long q_bs,
                          long k_bs, long v_bs, long o_bs, long do_bs, long dq_bs, long dk_bs,
                          long dv_bs, int strict, void* stream);
int pg_causal_attn_bwd_dkv(const float* q, const float* k, const float* v, const float* o,
                           const float* d_o, const float* lse2, float* delta, float* dq, float* dk,
                           float* dv, int N, int heads, int L, int dk_dim, int dv_dim, long q_bs,
                           long k_bs, long v_bs, long o_bs, long do_bs, long dq_bs, long dk_bs,
                           long dv_bs, int strict, void* stream);

/* Process-wide switch of the fused backward: enable = 1 / 0 sets it and returns the previous value,
 * enable < 0 only queries. The fused kernel sums dQ over key blocks in a timing-dependent order (last-bit
 * run-to-run differences in dQ); pg_attn_fused_bwd(0) selects the bit-reproducible two-kernel backward.
 * Initial value: 1, or the environment's PG_ATTN_FUSED_BWD at load time. */
int pg_attn_fused_bwd(int enable);

/* Host only, launches nothing: how the d_k = d_v = 4 matrix-core kernels (attention_mfma.hip) split a sequence of L
 * positions into blocks and hand them to the `waves` (1..8) waves of a workgroup; the launch reads the same plan.
 * which: 0 forward, 1 dQ (query blocks; a ragged L puts its short block FIRST), 2 dK/dV, 3 fused backward (64-key
 * blocks from 0). Entry e, wave by wave in the order a wave walks its list: block index, first row, 16-row groups
 * owned, wave, cost (group evaluations for which 0 / 1; 4 * rank + 5 for 2 / 3). The arrays hold ceil(L / 64)
 * entries. Returns the number of blocks, 0 if a wave's list would exceed 16 entries (the launch then leaves the
 * shape to the VALU kernels), PG_EINVAL for bad arguments. */
int pg_attn_block_plan(int which, int L, int waves, int* out_blk, int* out_q0, int* out_ngrp, int* out_wave,
                       int* out_cost);

/* Host only, launches nothing: which kernel family a pg_causal_attn_* launch of this problem takes and how it is laid out — the
 * answer of the one route function the launches themselves read (csrc/attention.hip: attn_route, which asks attention_mfma.hip and
 * attention_k4.hip in the launch's order). which: 0 forward, 1 dQ, 2 dK/dV, 3 the fused-backward request pg_causal_attn_bwd makes
 * first. flags: PG_ATTN_R_*, what the launch reads from its pointers and strides (a plane = the first image's first channel of the
 * tensor; a batch stride counts floats). The fused-backward switch (pg_attn_fused_bwd) is read, never changed. Fills
 * out[0 .. PG_ATTN_ROUTE_INTS):
 *   [0] family: PG_ATTN_FAM_VALU (attention.hip row-owner kernels), PG_ATTN_FAM_M44 (attention_mfma.hip, d_k = d_v = 4),
 *       PG_ATTN_FAM_K4 (attention_k4.hip); for which = 3 also PG_ATTN_FAM_DECLINED: no fused kernel takes it, the dQ and dK/dV
 *       launches follow (route them with which = 1, 2)
 *   [1] the fused-backward switch as found (0 / 1)
 *   [2] [3] [4] template instantiation: VALU Cfg<DK, DV> (head dims padded up), 0; k4 <DKT, DVT, QB> (d_k 4 -> DKT 1, else d_k / 4;
 *       DVT = d_v / 16; QB = 16-row groups per block, the fused k4 backward: key groups per block); M44 4, 4, 0
 *   [5] [6] [7] grid x, y, z   [8] block size   [9] dynamic LDS bytes
 *   [10] VALU: 64-row blocks per workgroup (<= 16)   [11] VALU: rows per LDS tile, kt (which 0, 1) resp. kt2 (which 2)
 *   [12] VALU: LDS tiles a sequence of L rows spans, ceil(L / [11])
 *   [13] waves per workgroup   [14] M44: LDS plane stride lp in floats   [15] M44: float4 stores (L % 4 == 0, planes aligned)
 *   [16] M44 variant: which 2: 1 = bf16x3 score tile; which 3: the kernel's compile-time plane stride (848, 1040, or 0 = any)
 * Fields that do not apply to the family are 0. d_k = d_v = 4 stays on the matrix cores only while the kernel's LDS planes fit 160 KB,
 * kernel by kernel: fused backward L <= 1792, dQ L <= 1984, dK/dV L <= 2240, forward L <= 3392 (L rounded up to 64); beyond, that
 * kernel alone runs on the VALU family, so one forward / backward may mix the two (they share lse2 and delta).
 * Returns 0, or the status the launch would return (PG_ESHAPE: no kernel instantiates the head dims at this L; out holds
 * [0] = PG_ATTN_FAM_NONE, [1] and zeros; head dims above 64: out untouched); PG_EINVAL for a null pointer, a short array, a bad `which` or a non-positive dimension. */
#define PG_ATTN_R_QKV_MISALIGNED 1     /* q, k or v is not 16-byte aligned */
#define PG_ATTN_R_O_MISALIGNED 2       /* the forward's o is not 16-byte aligned */
#define PG_ATTN_R_GRADIN_MISALIGNED 4  /* d_o, lse2 or delta of a backward launch is not 16-byte aligned */
#define PG_ATTN_R_DQ_MISALIGNED 8      /* dq is not 16-byte aligned */
#define PG_ATTN_R_DKV_MISALIGNED 16    /* dk or dv is not 16-byte aligned */
#define PG_ATTN_R_QKV_STRIDE 32        /* q_bs, k_bs or v_bs is not a multiple of 4 */
#define PG_ATTN_R_O_STRIDE 64          /* o_bs is not a multiple of 4 */
#define PG_ATTN_R_DO_STRIDE 128        /* do_bs is not a multiple of 4 */
#define PG_ATTN_R_DQ_STRIDE 256        /* dq_bs is not a multiple of 4 */
#define PG_ATTN_R_DKV_STRIDE 512       /* dk_bs or dv_bs is not a multiple of 4 */
#define PG_ATTN_FAM_VALU 0
#define PG_ATTN_FAM_M44 1
#define PG_ATTN_FAM_K4 2
#define PG_ATTN_FAM_DECLINED (-1)
#define PG_ATTN_FAM_NONE (-2)
#define PG_ATTN_ROUTE_INTS 17
int pg_attn_route(int which, int N, int heads, int L, int dk, int dv, int flags, int* out, int n_out);

/* ---------------------------------------------------------------------------------------
 * Linear causal attention (O(L) memory).  nn/attention.py:168-195 (_UnnormalizedLinearCausalAttention
 * forward / backward: the per-position loops) and :256-275 (LinearCausalAttention.forward):
 *   num[l] = phi(q[l]) . sum_{j <= l} phi(k[j])^T v[j]            (inclusive of j = l)
 *   den[n,h,l] = 1 / (sum_i phi(q)[n,h,l,i] * sum_{h' <= h} phi(k)[n,h',l,i] + 1e-10)
 *   out = num * den
 * The denominator's cumsum runs over the HEADS axis, as the reference's
 * einsum("nlhi,nlhi->nlh", Q, K.cumsum(1)) on (N, heads, L, d) tensors does (not causal over positions).
 * q: (N, heads*dk, L), k / v: views of the _kv output (N, heads*dk + heads*dv, L), out: (N, heads*dv, L);
 * head h owns channels [h*d, (h+1)*d) (_to_multihead). *_bs = batch stride in floats (k, v, dk, dv share
 * kv_bs; g shares o_bs; dq shares q_bs). den: (N, heads, L), written by _fwd, read by _bwd.
 * feature: PG_FEATURE_ELU1 applies phi = elu + 1 to q and k inside the kernels (the reference's default
 * feature_fn; the backward recomputes phi and phi' from the raw q, k); PG_FEATURE_IDENTITY takes q and k as
 * already mapped (a custom feature_fn applied by the caller). Chunked prefix-state scans on fp32 MFMAs
 * (linear_attention.hip); deterministic (no atomics). dk, dv in [1, 64] (PG_ESHAPE otherwise), any L >= 1.
 * ws: workspace of pg_linear_attn_workspace_floats(..., backward) floats, caller-allocated (0 floats: may be NULL).
 * _bwd writes dq, dk, dv (not accumulated).
 * ------------------------------------------------------------------------------------- */
#define PG_FEATURE_IDENTITY 0
#define PG_FEATURE_ELU1 1
size_t pg_linear_attn_workspace_floats(int N, int heads, int L, int dk, int dv, int backward);
int pg_linear_attn_fwd(const float* q, const float* k, const float* v, float* out, float* den, float* ws,
                       size_t ws_floats, int N, int heads, int L, int dk, int dv, long q_bs, long kv_bs,
                       long o_bs, int feature, void* stream);
int pg_linear_attn_bwd(const float* q, const float* k, const float* v, const float* out, const float* den,
                       const float* g, float* dq, float* dk, float* dv, float* ws, size_t ws_floats, int N,
                       int heads, int L, int dk_dim, int dv_dim, long q_bs, long kv_bs, long o_bs, int feature,
                       void* stream);

/* ---------------------------------------------------------------------------------------
 * MaskedLinear / MADE (models/autoregressive/made.py:21-33: `self.weight.data *= self.mask` then
 * nn.Linear.forward; :39-145: the masks MADE draws from integer "degrees", _sample_masks :71-102).
 * x: (N, in), w: (out, in), b: (out), y / dy: (N, out), dx: (N, in), all dense row-major.
 * The mask is M[o][i] = deg_in[i] <= deg_out[o] (strict != 0: deg_in[i] < deg_out[o], MADE's output layer),
 * evaluated from the two int32 degree vectors (device, lengths in / out) inside the kernels: no dense mask is
 * read. deg_in = deg_out = NULL: unmasked (plain F.linear); exactly one of them NULL: PG_EINVAL.
 * Masked GEMMs on v_mfma_f32_16x16x4_f32 (masked_linear.hip): fp32-exact, deterministic (no atomics). _fwd / _dgrad
 * split k when the output has too few tiles to fill the chip; ws is then a caller-allocated workspace of
 * pg_masked_linear_workspace_floats(N, in, out, dgrad) floats (0 floats: no split, ws may be NULL).
 * Any N, in, out >= 1 (PG_ESHAPE otherwise, and for N or out above 65535 * 64).
 *  _fwd    y = x (w o M)^T + b (b may be NULL), relu != 0 fuses nn.ReLU into the epilogue; with degrees it also
 *          writes w o M back into w (the reference's in-place masking; made.py:32).
 *  _dgrad  dx = dy (w o M), times (relu_out > 0) if relu_out (N, in) is given: the ReLU' of the PREVIOUS layer,
 *          whose stored output is this layer's input (nn.ReLU's backward, made.py:63). dx is written.
 *  _wgrad  dw += dy^T x, db += sum_n dy (db may be NULL): the UNMASKED weight gradient of the reference (the mask
 *          is applied to weight.data outside autograd); the results are ADDED (gradient sinks / zeroed buffers).
 *  _mask   mask = M as 0. / 1. floats (out, in): the layer's `mask` buffer (made.py:24, set_mask :27-28).
 * ------------------------------------------------------------------------------------- */
size_t pg_masked_linear_workspace_floats(int N, int in, int out, int dgrad);
int pg_masked_linear_fwd(const float* x, float* w, const float* b, const int* deg_in, const int* deg_out, int strict,
                         float* y, int N, int in, int out, int relu, float* ws, size_t ws_floats, void* stream);
int pg_masked_linear_dgrad(const float* dy, const float* w, const int* deg_in, const int* deg_out, int strict,
                           const float* relu_out, float* dx, int N, int in, int out, float* ws, size_t ws_floats,
                           void* stream);
int pg_masked_linear_wgrad(const float* x, const float* dy, float* dw, float* db, int N, int in, int out,
                           void* stream);
int pg_masked_linear_mask(float* mask, const int* deg_in, const int* deg_out, int strict, int in, int out,
                          void* stream);

/* ---------------------------------------------------------------------------------------
 * Sampling a one-hidden-layer MADE in one launch on cached hidden sums (csrc/made_sample.hip; the reference's sampler,
 * made.py:125-141, runs one full forward per dimension). All tensors dense row-major fp32; w1 (H, D) and w2 (D, H) are the
 * layers' weights ALREADY masked (exact zeros where the mask is 0: the kernels evaluate no mask).
 * Per sample n, a[h] = b1[h]; then for i = order[0], order[1], ..., order[D - 1]:
 *   l = b2[i] + sum_h max(a[h], 0) * w2[i][h];  p = 1 / (1 + exp(-l));
 *   x = canvas[n][i] if that is >= 0 (any float, not only 0 and 1), else (uniforms[n][i] < p ? 1 : 0);
 *   canvas[n][i] = x;  logits_out[n][i] = l (logits_out may be NULL);  a[h] += x * w1[h][i] for every h.
 * order: int32 (D), a permutation of 0..D-1 (an entry outside [0, D) is clamped into it); canvas, uniforms, logits_out: (N, D),
 * uniforms indexed by dimension, not by step. All arithmetic fp32; no float atomics, the sum over h in a fixed order that
 * depends on H alone: a sample's rows of canvas and logits_out are bit-identical from run to run and for any N.
 * pg_made_sample_plan (host only, no device call) is the one function that decides the domain and the geometry; the pack and
 * the launch call it too. It fills out[0 .. PG_MADE_SAMPLE_PLAN_INTS): samples per workgroup, threads per workgroup, hidden
 * units per thread, LDS bytes per workgroup, pack floats, floats of a padded weight row (threads * units), workgroups, the
 * largest H. Any D, N >= 1 and H in 1..8192 with a pack below 2^31 floats (PG_ESHAPE otherwise, from the plan, the pack and
 * the launch alike, nothing launched); PG_EINVAL for a null pointer, a short array, a non-positive dimension or a pack that
 * is not 16-byte aligned.
 *   pg_made_sample_pack: pack (D, 2, row floats) = [w2[i][:] | w1[:][i]] per dimension i, zeros from H on: what a step reads,
 *   contiguous. Made once per call from the masked weights.
 * ------------------------------------------------------------------------------------- */
#define PG_MADE_SAMPLE_PLAN_INTS 8
int pg_made_sample_plan(int D, int H, int N, int* out, int out_len);
int pg_made_sample_pack(const float* w1, const float* w2, float* pack, int D, int H, void* stream);
int pg_made_sample(const float* pack, const float* b1, const float* b2, const int* order, float* canvas,
                   const float* uniforms, float* logits_out, int N, int D, int H, void* stream);

/* ---------------------------------------------------------------------------------------
 * NADE (reference models/autoregressive/nade.py:42-68) as a chunked prefix scan, forward and backward (csrc/nade.hip). All
 * tensors dense row-major fp32: x, probs, logits, g (N, D); in_w (H, D), in_b (H), h_w (D, H), h_b (D). Per sample n,
 * a_0 = in_b; then for i = 0 .. D - 1:  l_i = h_b[i] + sum_h max(a_i[h], 0) h_w[i][h];  p_i = sigmoid(l_i);
 * a_{i+1}[h] = fma(x[n][i], in_w[h][i], a_i[h]). x is used as given (teacher forcing, any float).
 * pg_nade_plan (host only, no device call) is the one function that decides the domain and the geometry; both launches call
 * it too. It fills out[0 .. PG_NADE_PLAN_INTS): [0] the chunk length over D, [1] the chunks, [2] hidden units per forward
 * thread, [3] samples per forward workgroup, [4] H padded, [5] forward workgroups, [6] samples per backward tile, [7] partial
 * rows of the sums over samples, [8] sample tiles a backward workgroup loops over, [9] backward workgroups, [10] LDS bytes of
 * the largest kernel, [11] checkpoint floats = chunks * N * H padded (ckpt, and etot of the backward: per-sample tensors,
 * they grow with N as the activations do), [12] workspace floats of the partial rows (bounded by [13] rows whatever N is),
 * [13] the cap of the partial rows, [14] the largest H. Any D, N >= 1 and H in 1..8192 whose launches stay below 2^31
 * workgroups (PG_ESHAPE otherwise, from the plan and the launches alike, nothing launched); PG_EINVAL for a null pointer, a
 * short array or workspace, a non-positive dimension or checkpoints that are not 16-byte aligned.
 *   pg_nade_fwd: writes ckpt (chunks, N, H padded), the pre-activations a_{c T} at the chunk starts, then probs and logits.
 *   pg_nade_bwd: from g = dL/dprobs ADDS dL/d in_w, in_b, h_w, h_b into d_* (each may be NULL). It recomputes a_i inside a
 *   chunk from ckpt by the forward's own sequence of fused multiply-adds, so the ReLU mask is the forward's bit for bit
 *   (derivative 0 at 0). etot: scratch of checkpoint size. No gradient with respect to x.
 * No float atomics; every sum has an order that depends on (N, D, H) alone: outputs and gradients are bit-identical from run
 * to run, a sample's row of probs / logits also for any N. No host synchronisation (capturable).
 * ------------------------------------------------------------------------------------- */
#define PG_NADE_PLAN_INTS 15
int pg_nade_plan(int D, int H, int N, long long* out, int out_len);
int pg_nade_fwd(const float* x, const float* in_w, const float* in_b, const float* h_w, const float* h_b, float* ckpt,
                float* probs, float* logits, int N, int D, int H, void* stream);
int pg_nade_bwd(const float* x, const float* in_w, const float* h_w, const float* logits, const float* g, const float* ckpt,
                float* etot, float* d_in_w, float* d_in_b, float* d_h_w, float* d_h_b, int N, int D, int H, float* ws,
                size_t ws_floats, void* stream);

/* ---------------------------------------------------------------------------------------
 * Dense linear layers on large-tile fp32-MFMA GEMMs (csrc/dense_linear.hip): the coupling networks of NICE (reference
 * models/flow/nice.py). w (out, in) dense row-major; every activation operand is (N, columns) fp32 with a ROW STRIDE in floats
 * (ld >= columns), so one half of an (N, F) tensor is an operand as it lies.
 * pg_dense_linear_plan (host only, no device call) is the one function that decides the domain, the tile variant, the k-split
 * and the workspace; every launch calls it too. kind: PG_DENSE_FWD / _DGRAD / _WGRAD. It fills out[0 .. PG_DENSE_PLAN_INTS):
 * [0] the tile variant (0: 64 x 64 on v_mfma_f32_16x16x4_f32, 1: 128 x 128 on v_mfma_f32_32x32x2_f32), [1] tile rows, [2] tile
 * columns, [3] k per LDS chunk, [4] rows R, [5] columns C and [6] depth K of the product (forward N, out, in; data gradient
 * N, in, out; weight gradient out, in, N), [7] row tiles, [8] column tiles, [9] k slices, [10] k per slice, [11] GEMM
 * workgroups, [12] workgroups of the reduce launch (0 without a split), [13] the workspace floats (0 without a split).
 * The large tile is taken where it alone gives >= 192 workgroups; else the small one, split along k where it gives < 128
 * (at least two chunks per slice, at most 64 slices). Slices write raw partial sums to ws; a second launch adds them in slice
 * order and applies the epilogue. Any N, in, out in 1 .. 2^30 with at most 2^31 - 1 tiles: PG_ESHAPE otherwise, from the plan and the
 * launches alike; PG_EINVAL for a null operand, a row stride below the row length, a sign other than +1 / -1 or a short workspace.
 *   fwd:   y = x w^T + b (b may be NULL), then relu != 0: max(., 0); or with res != NULL: y = res + sign (x w^T + b), the
 *          additive coupling law (sign +1) and its inverse (-1); y may be res.
 *   dgrad: dx = sign (dy w), zeroed where relu_out <= 0 (relu_out, may be NULL: the stored ReLU output that was this layer's
 *          input), then + addend (may be NULL).
 *   wgrad: dw += sign dy^T x, db += sign sum_n dy (db may be NULL): added into flat-gradient sinks or zeroed buffers. With a
 *          k-split the batch is cut into slices whose partial dw and db are merged in slice order.
 * An fp32 MFMA is an fmaf chain in k order: every output element is owned by one lane and summed in an order fixed by the
 * shape. No float atomics, bit-identical from run to run, no host synchronisation (capturable).
 * pg_nice_scale_fwd: z = y exp(sign s), s (F) over dense (N, F). _bwd: dy = dz exp(sign s) (dy may be NULL) and
 *   ds[j] += sign sum_n dz[n][j] z[n][j] (ds may be NULL) through pg_nice_scale_bwd_workspace_floats floats of partial rows
 *   (at most 64) merged in row order.
 * pg_logistic_logprob_fwd: lp[n] = -sum_j (|z| + 2 log1p(exp(-|z|))) = sum_j -(softplus(z) + softplus(-z)) over dense (N, F),
 *   one workgroup per sample, a fixed order. _bwd: dz[n][j] = -g[n] tanh(z[n][j] / 2).
 * ------------------------------------------------------------------------------------- */
#define PG_DENSE_FWD 0
#define PG_DENSE_DGRAD 1
#define PG_DENSE_WGRAD 2
#define PG_DENSE_PLAN_INTS 14
int pg_dense_linear_plan(int N, int in, int out, int kind, long long* outv, int out_len);
int pg_dense_linear_fwd(const float* x, long ldx, const float* w, const float* b, const float* res, long ldres, int sign, float* y,
                        long ldy, int N, int in, int out, int relu, float* ws, size_t ws_floats, void* stream);
int pg_dense_linear_dgrad(const float* dy, long lddy, const float* w, const float* relu_out, long ldrelu, const float* addend,
                          long ldadd, int sign, float* dx, long lddx, int N, int in, int out, float* ws, size_t ws_floats,
                          void* stream);
int pg_dense_linear_wgrad(const float* x, long ldx, const float* dy, long lddy, int sign, float* dw, float* db, int N, int in, int out,
                          float* ws, size_t ws_floats, void* stream);
int pg_nice_scale_fwd(const float* y, const float* s, float* z, int N, int F, int sign, void* stream);
size_t pg_nice_scale_bwd_workspace_floats(int N, int F);
int pg_nice_scale_bwd(const float* dz, const float* z, const float* s, float* dy, float* ds, int N, int F, int sign, float* ws,
                      size_t ws_floats, void* stream);
int pg_logistic_logprob_fwd(const float* z, float* lp, int N, int F, void* stream);
int pg_logistic_logprob_bwd(const float* z, const float* g, float* dz, int N, int F, void* stream);

/* ---------------------------------------------------------------------------------------
 * The Fully Visible Belief Network (reference models/autoregressive/fvbn.py) on packed triangular storage (csrc/fvbn.hip):
 * logits[n][i] = b[i] + sum_{j < i} W[i][j] x[n][j]. x, dy, logits, canvas, uniforms: dense row-major fp32 (N, D); b, db (D).
 * PACKED weight wp (P(D) floats, 16-byte aligned): row i of the strictly lower triangle holds len(i) = max(1, i) values (row 0:
 * the reference's dummy weight, multiplied by a zero input there and never read here), then zeros up to pad(i) =
 * roundup(len(i), 4) floats; off(i) = sum_{k < i} pad(k) = pg_fvbn_row_offset(i) (-1 for i < 0), P(D) = off(D).
 * pg_fvbn_plan (host only, no device call) is the one function that decides the domain and every geometry; every launch calls
 * it too. It fills out[0 .. PG_FVBN_PLAN_INTS): [0] P(D), [1] the tile edge (64: rows and columns of an output tile, on
 * v_mfma_f32_16x16x4_f32), [2] k per LDS chunk, [3] tiles along D, [4] forward tiles along N, [5] forward workgroups,
 * [6] (column tile, k chunk) pairs the forward multiplies, [7] weight-gradient tiles (tile column <= tile row), [8] slices
 * along N of the weight gradient (more than one where [7] < 128; at least two chunks each, at most 64), [9] samples per slice,
 * [10] weight-gradient workgroups, [11] workgroups of its merge launch (0 without a split), [12] workspace floats (0 without a
 * split), [13] samples per sampler workgroup, [14] sampler workgroups, [15] sampler LDS bytes, [16] the largest D, [17] k chunks
 * of a forward slice, [18] forward slices over all column tiles, [19] 1 where the forward is split along k (fewer than 128
 * output tiles and a column tile with more than one slice: [5] is then slices x tiles along N), [20] workgroups of its merge
 * launch and [21] its workspace floats (both 0 without a split).
 * D in 1 .. 8192, N in 1 .. 2^30 with fewer than 2^31 forward workgroups: PG_ESHAPE otherwise, from the plan and the launches
 * alike, nothing launched. PG_EINVAL for a null pointer, a short array or workspace and a wp that is not 16-byte aligned.
 * pg_fvbn_tiles (host only) lists, for the forward (kind PG_FVBN_TILES_FWD: the (column tile, k chunk) pairs) or the weight
 * gradient (PG_FVBN_TILES_WGRAD), the rectangles [i0, i1) x [j0, j1) of W the launch visits, 4 integers each, into out (at most
 * cap rectangles are written; *count is their number): together they hold every (i, j < i) exactly once.
 *   fwd:    only k chunks at or below the diagonal are multiplied; a weight at j >= i is a zero formed by a predicate, the
 *           16-byte loads stay inside row i's own storage. x is used AS GIVEN and finite values are assumed: the reference never
 *           reads x[:, j >= i], here such entries meet exact zeros, so a NaN or infinity there would spread.
 *           logits[:, 0] = b[0] bit for bit. The sum over j: an fmaf chain per slice of [17] chunks, the slices added in
 *           ascending order, then b; with a split the slices are workgroups of their own and a second launch adds their
 *           partial sums from ws in that order: the same bits with and without a split.
 *   wgrad:  ADDS dwp[off(i) + j] += sum_n dy[n][i] x[n][j] for j < i only and db[i] += sum_n dy[n][i] (either may be NULL):
 *           into flat-gradient sinks or zeroed buffers. Pads and row 0 are not written (their gradient is exactly zero). With
 *           a split the slices' partial sums go to ws and a second launch adds them in slice order. No data gradient.
 *   sample: per sample, i = 0 .. D - 1: l = b[i] + sum_{j < i} wp[off(i) + j] x_j; x_i = canvas[n][i] where that is >= 0, else
 *           1 if uniforms[n][i] < sigmoid(l), else 0; writes canvas and, if logits_out is not NULL, logits_out[n][i] = l.
 *           One launch for the whole batch.
 *   pack:   dense (D, D) -> packed: the strict lower triangle, row 0's dummy value from [0][0], zero pads. unpack: the inverse,
 *           zeros on and above the diagonal except [0][0].
 * An fp32 MFMA is an fmaf chain in k order; every sum has an order fixed by the shape (the sampler's by i alone), no float
 * atomics: bit-identical from run to run, a sample's row of logits for any N and any slot. No host synchronisation (capturable).
 * ------------------------------------------------------------------------------------- */
#define PG_FVBN_PLAN_INTS 22
#define PG_FVBN_TILES_FWD 0
#define PG_FVBN_TILES_WGRAD 1
long long pg_fvbn_row_offset(int i);
int pg_fvbn_plan(int D, int N, long long* out, int out_len);
int pg_fvbn_tiles(int D, int kind, long long* out, long long cap, long long* count);
int pg_fvbn_fwd(const float* x, const float* wp, const float* b, float* logits, int N, int D, float* ws, size_t ws_floats, void* stream);
int pg_fvbn_wgrad(const float* x, const float* dy, float* dwp, float* db, int N, int D, float* ws, size_t ws_floats, void* stream);
int pg_fvbn_sample(const float* wp, const float* b, float* canvas, const float* uniforms, float* logits_out, int N, int D,
                   void* stream);
int pg_fvbn_pack(const float* dense, float* wp, int D, void* stream);
int pg_fvbn_unpack(const float* wp, float* dense, int D, void* stream);

/* ---------------------------------------------------------------------------------------
 * The dense symmetric solve of a Gaussian process (reference models/gaussian_process.py; csrc/gp.hip): squared-exponential
 * covariance, a blocked right-looking fp32 Cholesky factorisation that can be appended to, the triangular solves and the
 * strided GEMM update they are built from. Everything is fp32; EVERY operand is a row-major matrix with a leading dimension in
 * floats (ld >= its columns), so a factor lives in a buffer larger than itself.
 * pg_gp_plan (host only, no device call) is the one function that decides the domain and the geometry; every entry point calls
 * it too (with 1 for the dimensions it does not have). It fills out[0 .. PG_GP_PLAN_INTS): [0] the panel width and tile edge
 * (64, on v_mfma_f32_16x16x4_f32), [1] k per LDS chunk, [2] panels of n, [3] row tiles of m, [4] the covariance route (0: exact
 * differences on the VALU, 1: |a|^2 + |b|^2 - 2 a.b with the cross term on the MFMA), [5] the largest d of route 0, [6] the
 * tiles the symmetric covariance computes (on or below the diagonal), [7] the tiles of the cross covariance, [8] the launches
 * of a full factorisation (3 panels - 2), [9] of a forward solve over n columns (2 panels - 1), [10] the workgroups of the
 * first trailing update, [11] the largest n and m, [12] the largest d, [13] the largest p, [14] row tiles of p, [15] the
 * largest d route 0 holds when it is forced.
 * n, m in 1 .. 16384 (element offsets fit 32 bits), d in 1 .. 4096, p (columns of y) in 1 .. 4096: PG_ESHAPE otherwise, from
 * the plan and the launches alike, nothing launched. PG_EINVAL for a null pointer, a short array, a row stride below the row
 * length, unknown flags. Without a device an entry point returns hipErrorNoDevice (100), and only after the plan and the
 * argument checks accepted the call.
 *   se_kernel:  pg_gp_stat_kernel (below) with kind SE and no inv_ls, under its own name in the messages.
 *               K[i][j] = std^2 exp(-|a_i - b_j|^2 / (2 lengthscale^2)) for a (n, d), b (m, d) into K (n, m). PG_GP_LOWER: only
 *               elements with j <= i + diag_off are written and tiles wholly above that line are not visited; PG_GP_DIAG: the
 *               elements j == i + diag_off are written as exactly std^2 + noise_var; PG_GP_MIRROR (a is b, lower, diag_off 0):
 *               K[j][i] = K[i][j] as well, so the matrix is exactly symmetric. Route 1 clamps the squared distance at 0 before
 *               the exp. PG_GP_SE_DIRECT / PG_GP_SE_MFMA force a route (route 0: d <= 64, PG_ESHAPE above). An element's bits
 *               depend on its two rows alone, not on n, m or the tile it lies in.
 *   add_diag:   A[i][i] += value for i < n.
 *   gemm_nt:    C (R, C) = C - A B^T (PG_GP_PLUS: + A B^T) over k < K, A (R, K), B (C, K); PG_GP_B_TRANS: B is read as (K, C),
 *               the A B form. The accumulators are SEEDED with the tile of C and the product is subtracted inside the MFMA chain:
 *               an element is fmaf(-a_k, b_k, .) in ascending k starting from C's value, so an update applied panel after
 *               panel is one continuous chain, whatever the blocking. PG_GP_LOWER: only elements with c <= r + diag_off are
 *               read and written; PG_GP_MIRROR (square, lower, diag_off 0): C[c][r] = C[r][c] too. No k-split.
 *   potrf_diag: the unblocked lower Cholesky of one diagonal block (jb <= 64 rows) in place on the VALU; rows < done are
 *               final and untouched, rows >= done continue from the values the updates left. A pivot that is not > 0 (a NaN
 *               included) stores base + index + 1 into *info by a plain store, only while *info is 0; the kernel goes on.
 *   trsm_diag:  X L_kk^T = B in place (transposed != 0: X L_kk = B) for rows x jb, 64 rows per workgroup; columns < done are
 *               final (forward form). fmaf chains in ascending (transposed: descending) k, then one IEEE division. The kernel
 *               (gp_subst_diag_kernel, csrc/gp_common.h) is also trtri_t's substitution.
 *   potrf:      the lower factor of A (n, n) in place, right-looking, at most three launches per panel of 64 columns; the strict
 *               upper triangle is neither read nor written. n_done > 0: rows < n_done hold a finished factor and only rows
 *               n_done .. n (holding A's values in columns 0 .. their own) are completed; the result has the bits of the full
 *               factorisation. *info as in potrf_diag (the caller zeroes it).
 *   trsm_right: X L^T = B in place for X (rows, n) (transposed != 0: X L = B), right-looking; col_done > 0 (forward only):
 *               columns < col_done are final, the others hold B.
 * No float atomics, no host synchronisation (capturable), bit-identical from run to run.
 * ------------------------------------------------------------------------------------- */
#define PG_GP_PLAN_INTS 16
#define PG_GP_LOWER 1
#define PG_GP_MIRROR 2
#define PG_GP_DIAG 4
#define PG_GP_PLUS 8
#define PG_GP_B_TRANS 16
#define PG_GP_SE_DIRECT 32
#define PG_GP_SE_MFMA 64
int pg_gp_plan(int n, int m, int d, int p, long long* out, int out_len);
int pg_gp_se_kernel(const float* a, long lda, int n, const float* b, long ldb, int m, int d, float std, float lengthscale,
                    float noise_var, float* k, long ldk, int diag_off, int flags, void* stream);
int pg_gp_add_diag(float* a, long ld, int n, float value, void* stream);
int pg_gp_gemm_nt(const float* a, long lda, const float* b, long ldb, float* c, long ldc, int R, int C, int K, int diag_off, int flags,
                  void* stream);
int pg_gp_potrf_diag(float* a, long ld, int jb, int done, int base, int* info, void* stream);
int pg_gp_trsm_diag(const float* l, long ld, float* x, long ldx, int rows, int jb, int done, int transposed, void* stream);
int pg_gp_potrf(float* a, long ld, int n, int n_done, int* info, void* stream);
int pg_gp_trsm_right(const float* l, long ld, int n, float* x, long ldx, int rows, int col_done, int transposed, void* stream);

/* ---------------------------------------------------------------------------------------
 * The log marginal likelihood of a Gaussian process and its gradients with respect to the hyperparameters (csrc/gp_mll.hip),
 * from the cached factor K = K_f + noise_var I = L L^T, z^T = (L^-1 r)^T (p, n) and alpha^T = (K^-1 r)^T (p, n), r = y - value:
 *     log p(y) = -1/2 sum z^2 - p sum_i log L_ii - (n p / 2) log 2 pi,      G = alpha alpha^T - p K^-1,
 *     d/d std = sum_ij G_ij K_f,ij / std,   d/d lengthscale = sum_ij G_ij K_f,ij D2_ij / (2 l^3),   d/d noise_var = tr G / 2,
 *     d/d value = sum alpha.
 * K^-1 = X X^T with X = L^-T UPPER triangular, so every product is triangular: about n^3 / 3 flops for X and for X X^T each.
 * Operands as above (fp32, row-major, leading dimension in floats). pg_gp_mll_plan (host only) is the one function that decides
 * the domain — that of pg_gp_plan: n in 1 .. 16384, d, p in 1 .. 4096 — and the geometry; every entry point below calls it and
 * follows the status conventions above (PG_ESHAPE, PG_EINVAL, hipErrorNoDevice only for an accepted call). It fills
 * out[0 .. PG_GP_MLL_PLAN_INTS): [0] the tile edge (64), [1] panels P of n, [2] the launches of the inverse (2 P - 1), [3] the
 * 64x64x64 tile-products of the inverse on the MFMA (sum_k (k + 1)(P - 1 - k)), [4] the tiles X X^T writes (on or below the
 * diagonal, P (P + 1) / 2), [5] its tile-products (sum_I (I + 1)(P - I): tile (I, J) starts its k loop at row tile I), [6] the
 * tiles the reduction visits (P (P + 1) / 2), [7] its partial rows (one per tile, three floats each), [8] the workspace floats
 * the caller passes to se_mll_sums (3 x [7]), [9] the covariance route of the reduction (that of pg_gp_plan: 0 exact
 * differences, 1 the MFMA), [10] the largest d of route 0, [11] the largest n, [12] d, [13] p, [14] the k chunks of the outer
 * product alpha_i . alpha_j (every p takes the in-kernel MFMA route), [15] the launches of the reduction (2).
 *   trtri_t:     X = L^-T into the upper triangle of x (diagonal included); the strict lower triangle of x and the strict upper
 *                triangle of l are neither read nor written; x must not be l. The right-looking solve of X L^T = I in panels
 *                at absolute multiples of 64: panel k is solved for the rows above its end only (rows below are zero) by the
 *                fmaf chain in ascending k and one IEEE division on the VALU (no explicit inverse of a diagonal block beyond
 *                the block's own result), then the (k + 1) x (P - 1 - k) tiles to its right are updated on the MFMA, the
 *                accumulators seeded with x (zero where a tile is touched first).
 *   gram_upper:  H = X X^T for the upper triangular X, on the lower triangle of h (diagonal included); flags = PG_GP_MIRROR:
 *                h[j][i] = h[i][j] too. Tile (I, J), J <= I, starts its k loop at 64 I; the strict lower triangle of x is
 *                not read. Each element is one fmaf chain in ascending k. No k-split. h must not be x.
 *   se_mll_sums: pg_gp_stat_mll_sums (below) with kind SE, under its own name in the messages: one workgroup per 64 x 64 tile
 *                on or below the diagonal recomputes D2 and K_f from the rows of x (n, d) (the routes and the bits of
 *                se_kernel; the diagonal is K_f = std^2, D2 = 0 exactly), forms G_ij = sum_c alpha_ic alpha_jc - p H_ij in
 *                registers (only the lower triangle of h is read) and sums G K_f, G K_f D2 (off-diagonal elements twice) and
 *                G_ii; K_f, D2 and G are never written. Every workgroup writes its three fp32 partials into ws (ws_floats >=
 *                plan[8], PG_EINVAL below); a second launch of one workgroup adds them in double — thread t the tiles t, t +
 *                256, ... ascending, then a fixed tree — and writes out[0 .. 3) = d/d std, d/d lengthscale, d/d noise_var.
 *                lengthscale > 0, std != 0.
 *   mll_value:   one workgroup, fixed order, double accumulators: out[0] = log p(y), out[1] = sum alpha.
 * out is device memory. No float atomics, no allocation, no host synchronisation (capturable), bit-identical from run to run.
 * ------------------------------------------------------------------------------------- */
#define PG_GP_MLL_PLAN_INTS 16
int pg_gp_mll_plan(int n, int d, int p, long long* out, int out_len);
int pg_gp_trtri_t(const float* l, long ld, int n, float* x, long ldx, void* stream);
int pg_gp_gram_upper(const float* x, long ldx, int n, float* h, long ldh, int flags, void* stream);
int pg_gp_se_mll_sums(const float* x, long ldx, int n, int d, float std, float lengthscale, const float* h, long ldh,
                      const float* alpha_t, long lda, int p, float* ws, size_t ws_floats, float* out, void* stream);
int pg_gp_mll_value(const float* l, long ld, int n, const float* zt, long ldz, const float* alpha_t, long lda, int p, float* out,
                    void* stream);

/* ---------------------------------------------------------------------------------------
 * Stationary kernels with per-dimension (ARD) lengthscales (csrc/gp.hip, csrc/gp_mll.hip). With w_c = 1 / l_c, s_c = a_c - b_c
 * and r^2 = sum_c (s_c w_c)^2 the covariance is k(a, b) = std^2 phi(r), and omega = -phi'(r) / r is finite at r = 0:
 *     PG_GP_KIND_SE        phi = exp(-r^2 / 2)                               omega = exp(-r^2 / 2)
 *     PG_GP_KIND_MATERN32  phi = (1 + sqrt(3) r) exp(-sqrt(3) r)             omega = 3 exp(-sqrt(3) r)
 *     PG_GP_KIND_MATERN52  phi = (1 + sqrt(5) r + 5 r^2 / 3) exp(-sqrt(5) r) omega = (5 / 3)(1 + sqrt(5) r) exp(-sqrt(5) r)
 * so that d k / d l_c = std^2 omega(r) s_c^2 / l_c^3 and, with G = alpha alpha^T - p K^-1 as above,
 *     d/d l_c = S_c / (2 l_c),  S_c = sum_ij G_ij std^2 omega(r_ij) ((x_ic - x_jc) w_c)^2;   shared l: sum_ij G_ij std^2 omega r^2 / (2 l).
 * Any other kind is PG_EINVAL. Status conventions as above.
 *   stat_kernel:   pg_gp_se_kernel's arguments, flags, routes (pg_gp_plan decides) and promises — the diagonal exactly
 *                  std^2 + noise_var, an element's bits a function of its two rows and of w alone — plus the kind and inv_ls, a
 *                  DEVICE pointer to the d floats w_c. inv_ls == NULL: the shared scalar `lengthscale` is used (kind SE is then
 *                  what pg_gp_se_kernel forwards to); otherwise the scalar is ignored. Route 0 forms (a_c - b_c) w_c, the
 *                  difference first: inputs far from the origin lose nothing and a duplicated row gives r = 0, phi = 1 exactly.
 *                  Route 1 scales the rows by w WHILE STAGING them into LDS (no extra launch, no scaled copy of the rows) and
 *                  clamps the squared distance at 0 before the square root.
 *   stat_mll_sums: pg_gp_se_mll_sums for any kind with one shared lengthscale, same arguments, domain and outputs; kind SE is
 *                  what pg_gp_se_mll_sums forwards to. The other kinds sum G std^2 omega r^2 directly.
 *   ard_mll_sums:  out[0 .. d + 2) = d/d std, d/d noise_var, d/d l_0 .. d/d l_{d-1}. One workgroup per 64 x 64 tile on or below
 *                  the diagonal forms G in registers (alpha_i . alpha_j on the MFMA for every p, only the lower triangle of h is
 *                  read, off-diagonal elements count twice). The per-dimension terms are exact differences on the VALU for
 *                  every d of the domain: the rows of x go through LDS in chunks of at most 64 columns, twice — first for r^2
 *                  (the ascending-c sum of the squares; not the bits of stat_kernel's route 1), then for the sums — once if
 *                  d <= 64. A workgroup writes one partial row of d + 2 fp32 values into ws (ws_floats >= plan[3]); a second
 *                  launch of d + 2 workgroups adds each column in double — thread t the tiles t, t + 256, ... ascending, then
 *                  the fixed tree — and applies 1 / std, 1 / 2 and 1 / (2 l_c). std != 0.
 * pg_gp_ard_plan (host only) is the one function that decides the domain of ard_mll_sums: that of pg_gp_mll_plan and d <= 256
 * (PG_ESHAPE above: the VALU term count is n^2 d / 2). It fills out[0 .. PG_GP_ARD_PLAN_INTS): [0] the tile edge, [1] the tiles
 * and partial rows, [2] the floats of a partial row (d + 2), [3] the workspace floats ([1] x [2]), [4] the column chunks of x,
 * [5] the launches (2), [6] the largest d, [7] the columns of a chunk.
 * No float atomics, nothing of size (n, n) written, no allocation, no host synchronisation (capturable), bit-identical from run
 * to run.
 * ------------------------------------------------------------------------------------- */
#define PG_GP_KIND_SE 0
#define PG_GP_KIND_MATERN32 1
#define PG_GP_KIND_MATERN52 2
#define PG_GP_ARD_PLAN_INTS 8
int pg_gp_stat_kernel(int kind, const float* a, long lda, int n, const float* b, long ldb, int m, int d, float std, float lengthscale,
                      const float* inv_ls, float noise_var, float* k, long ldk, int diag_off, int flags, void* stream);
int pg_gp_stat_mll_sums(int kind, const float* x, long ldx, int n, int d, float std, float lengthscale, const float* h, long ldh,
                        const float* alpha_t, long lda, int p, float* ws, size_t ws_floats, float* out, void* stream);
int pg_gp_ard_plan(int n, int d, int p, long long* out, int out_len);
int pg_gp_ard_mll_sums(int kind, const float* x, long ldx, int n, int d, float std, const float* inv_ls, const float* h, long ldh,
                       const float* alpha_t, long lda, int p, float* ws, size_t ws_floats, float* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Density estimators (models/mixture_models.py, models/kde.py) on streaming log-density kernels (density.hip):
 * the pairwise log-density c[n][k] = sum_d f(x[n][d], theta[k][d]) is one or two fp32-MFMA GEMMs plus a per-column
 * constant, reduced by a running logsumexp over column tiles; nothing of size N x K (x F) is written to memory.
 * x / test: (N, F), parameters / train: (K, F), dense row-major. Deterministic (no atomics).
 * Any N, K, F >= 1 (PG_ESHAPE otherwise, and for N above 65535 * 64 or K above 65535 * 32). ws is a caller-allocated
 * workspace of the matching _workspace_floats() floats (a shorter one: PG_EINVAL).
 *  pg_mixture_fwd  lse[n] = logsumexp_k (log_softmax(mixture_logits)_k + log p_k(x_n)).
 *                  kind PG_MIXTURE_BERNOULLI: p1 = logits (K, F), p2 unused, log p_k(x) = sum_d x l - softplus(l)
 *                  (binary_cross_entropy_with_logits: real-valued x allowed);
 *                  kind PG_MIXTURE_GAUSSIAN: p1 = mean, p2 = log_std (diagonal normal).
 *                  mixture_logits all -inf gives lse = -inf (torch's log_softmax gives NaN there).
 *                  stats (N, 2) receives, per row, the running (max, sum) of the logsumexp relative to component 0:
 *                  what the backward needs (it never sees lse).
 *  pg_mixture_bwd  from x, the forward's stats and the upstream gradient g (N): the gradients of mixture_logits (K), p1
 *                  and p2 (K, F) are ADDED to d_logits / d1 / d2 (gradient sinks / zeroed buffers; each may be NULL).
 *                  The responsibilities are recomputed tile by tile; the Gaussian sums are formed from (x - mean).
 *                  No input gradient.
 *  pg_kde_gaussian out[n] = logsumexp_k (-|x_n - y_k|^2 / (2 h^2)) - (F/2 log 2 pi + F log h + log K)
 *                  (kde.py GaussianKernel.forward), as alpha x.y - alpha/2 |y|^2 - alpha/2 |x|^2 with alpha = 1 / h^2.
 *  pg_kde_parzen   out[n] = log(coef * #{k: |x_n[d] - y_k[d]| / h <= 0.5 for all d} / K) in the reference's fp32
 *                  order (kde.py ParzenWindowKernel.forward); coef = 1 / h^F as the caller computed it. count 0: -inf;
 *                  coef = inf (it overflowed): +inf if every window contains x_n, NaN otherwise, as the reference.
 * ------------------------------------------------------------------------------------- */
#define PG_MIXTURE_BERNOULLI 0
#define PG_MIXTURE_GAUSSIAN 1
size_t pg_mixture_workspace_floats(int kind, int N, int K, int F, int backward);
int pg_mixture_fwd(int kind, const float* x, const float* mixture_logits, const float* p1, const float* p2, float* lse,
                   float* stats, int N, int K, int F, float* ws, size_t ws_floats, void* stream);
int pg_mixture_bwd(int kind, const float* x, const float* mixture_logits, const float* p1, const float* p2,
                   const float* stats, const float* g, float* d_logits, float* d1, float* d2, int N, int K, int F,
                   float* ws, size_t ws_floats, void* stream);
size_t pg_kde_workspace_floats(int N, int K, int F);
int pg_kde_gaussian(const float* test, const float* train, float bandwidth, float* out, int N, int K, int F, float* ws,
                    size_t ws_floats, void* stream);
int pg_kde_parzen(const float* test, const float* train, float bandwidth, float coef, float* out, int N, int K, int F,
                  void* stream);

/* (N,2,H,W) pixel-coordinate encoding, nn/attention.py:37-57 (torch.arange(-.5,.5,1/h)). */
int pg_image_positional_encoding(float* out, int N, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------
 * Elementwise pieces of the path.
 * ------------------------------------------------------------------------------------- */
int pg_act_fwd(const float* x, float* y, size_t n, int act, void* stream);
/* dx = dy * act'(x) */
int pg_act_bwd(const float* x, const float* dy, float* dx, size_t n, int act, void* stream);
/* GatedActivation: x (N,2C,L) -> y (N,C,L).  nn/convolution.py:62-66 */
int pg_gated_fwd(const float* x, float* y, int N, int C, int L, int gate, void* stream);
int pg_gated_bwd(const float* x, const float* dy, float* dx, int N, int C, int L, int gate,
                 void* stream);
/* y = res + gate(x): GatedActivation followed by the block's residual add in one pass
 * (pixel_snail.py:55-56 `x + self._activation(out)`); L % 4 == 0, 16-byte aligned tensors. */
int pg_gated_fwd_res(const float* x, const float* res, float* y, int N, int C, int L, int gate,
                     void* stream);
/* dx = dy * act'(pre) with the derivative recovered from the activation's OUTPUT v = y - res
 * (res may be NULL): backward of the fused convolution epilogue y = act(conv + bias) + res
 * (pixel_snail.py:27-28,113-119). act = PG_ACT_ELU (v > 0 ? 1 : v + 1) or PG_ACT_RELU. */
int pg_act_bwd_from_out(const float* y, const float* res, const float* dy, float* dx, size_t n,
                        int act, void* stream);
/* out = a + b */
int pg_add(const float* a, const float* b, float* out, size_t n, void* stream);
/* out[i] = value: the zero fills of gradient sinks, loss scalars and the VD-VAE decoder's constant top input
 * (torch.zeros on the reference path, e.g. vd_vae.py:379 torch.zeros_like(...)); a kernel, not a memset node
 * (a hipMemset2DAsync node of a captured step went wrong from its second replay on: profiles/README.md round 4 item 12) */
int pg_fill(float* out, float value, size_t n, void* stream);
/* out[b * per + i] = sum_k rows[k][b * batch_strides[k] + i], b < n_batch, i < per, k < n_rows <= 32 (rows, batch_strides: HOST
 * arrays copied into the launch; batch_strides == NULL: every row dense, stride per): (a) the sum over the per-block KL terms of a
 * hierarchical VAE, vd_vae.py:400 `torch.stack(kl_divs).sum(dim=0)`, in one launch; (b) the gradient of a tensor with several
 * readers (autograd's chain of `add` kernels) in one launch, where a gradient may be a channel slice of a wider tensor (dense per
 * image, batch stride > per) */
int pg_sum_rows(const float* const* rows, const long* batch_strides, int n_rows, float* out, long n_batch, long per, void* stream);
/* y[n,i] = x[n,i] + p[i] (learned positional map, image_gpt.py:86,106); i < per */
int pg_add_bcast_fwd(const float* x, const float* p, float* y, int N, size_t per, void* stream);
/* dp[i] += sum_n dy[n,i] */
int pg_add_bcast_bwd(const float* dy, float* dp, int N, size_t per, void* stream);

/* BCE-with-logits summed over pixels, averaged over batch: image_gpt.py:158-162.
 * loss[0] += (1/N) * sum_{n,i} [max(z,0) - z*x + log1p(exp(-|z|))]  (loss zeroed by caller) */
int pg_bce_logits_fwd(const float* z, const float* x, float* loss, int N, size_t per,
                      void* stream);
/* dz = gscale[0] * (sigmoid(z) - x) / N */
int pg_bce_logits_bwd(const float* z, const float* x, const float* gscale, float* dz, int N,
                      size_t per, void* stream);

/* ---------------------------------------------------------------------------------------
 * VAE pieces (models/vae/vd_vae.py:224,256; models/vae/vaes.py:17-33; vae.py:91-93,149-159).
 * ------------------------------------------------------------------------------------- */
/* 2x2 average pool, stride 2: x (planes, 2*OH, 2*OW) -> y (planes, OH, OW); planes = N*C */
int pg_avgpool2_fwd(const float* x, float* y, int planes, int OH, int OW, void* stream);
int pg_avgpool2_bwd(const float* dy, float* dx, int planes, int OH, int OW, void* stream);
/* the same with a second gradient of the pooled tensor's INPUT added in (dx = 0.25 * expand(dy) + res): the input of an
 * encoder stack's AvgPool2d is also read by the decoder's top-down blocks (vd_vae.py:224, 141-189), whose gradients arrive
 * through pass-through aliases — no gradient-sum kernel of autograd */
int pg_avgpool2_bwd_res(const float* dy, const float* res, float* dx, int planes, int OH, int OW, void* stream);
/* nearest-neighbour x2 upsample: x (planes, IH, IW) -> y (planes, 2*IH, 2*IW) */
int pg_upsample2_fwd(const float* x, float* y, int planes, int IH, int IW, void* stream);
int pg_upsample2_bwd(const float* dy, float* dx, int planes, int IH, int IW, void* stream);
/* 2x2 phase split (space-to-depth) and its inverse: x (planes, 2H, 2W) <-> xs (4, planes, H, W),
 * xs[2*pr+pc][plane][r][c] = x[plane][2r+pr][2c+pc]. merge==0 writes xs, merge==1 writes x. */
int pg_phase_split2(float* x, float* xs, int planes, int H, int W, int merge, void* stream);
/* the same between x and FOUR separate phase tensors p[2*pr+pc] (planes, H, W) (HOST array of 4 device pointers): the four phase
 * convolutions of a 4x4 / stride-2 transposed convolution (vaes.py:228-235) write their own outputs, which are interleaved here
 * without a stacked copy; merge == 0 scatters x's gradient back into four tensors */
int pg_phase_merge4(float* x, float* const* p, int planes, int H, int W, int merge, void* stream);
/* The four 2x2 phase kernels of a 4x4 / stride-2 weight, out (4, Co, Ci, 2, 2) contiguous:
 *   transposed == 0 (Conv2d weight (Co, Ci, 4, 4), vaes.py:153-160):  out[2pr+pc][o][c][i][j] = w[o][c][2i+1-pr][2j+1-pc]
 *   transposed == 1 (ConvTranspose2d weight (Ci, Co, 4, 4), vaes.py:228-235): out[2pr+pc][o][c][i][j] = w[c][o][2(1-i)+1-pr][2(1-j)+1-pc]
 * A, B = the weight's first two dimensions. pg_phase_weights_bwd is the adjoint from four gradient tensors g[k] (Co, Ci, 2, 2)
 * (HOST array of 4 device pointers, a null entry = no gradient): dw = (accumulate ? dw : 0) + scatter(g). */
int pg_phase_weights(const float* w, float* out, int A, int B, int transposed, void* stream);
int pg_phase_weights_bwd(const float* const* g, float* dw, int A, int B, int transposed, int accumulate, void* stream);
/* Fused Gaussian head. q, p: (N, >=2C, L) conv outputs holding [mean | log_std] in channels
 * [0,C) / [C,2C), read in place through batch strides q_bs / p_bs (floats). eps, z: (N, C, L).
 *   mode 0: z = mu_q + exp(s_q) eps ; kl[n] += sum KL(q || N(0,1))       (vae.py:91-93)
 *   mode 1: z = mu_q + exp(s_q) eps ; kl[n] += sum KL(q || p)            (vd_vae.py:177-186)
 *   mode 2: z = mu_p + exp(s_p) eps (sampling from the prior, no KL)     (vd_vae.py:166-168)
 * kl (N floats) is accumulated: the caller zeroes it. */
int pg_gauss_head_fwd(const float* q, const float* p, const float* eps, float* z, float* kl, int N,
                      int C, int L, long q_bs, long p_bs, int mode, void* stream);
/* dq / dp receive the gradient of the [mean | log_std] channels (written, not accumulated);
 * dz: (N,C,L) or NULL, dkl: (N) or NULL. */
int pg_gauss_head_bwd(const float* q, const float* p, const float* eps, const float* dz,
                      const float* dkl, float* dq, float* dp, int N, int C, int L, long q_bs,
                      long p_bs, int mode, void* stream);
/* out[0] += mean(v[0..n)) ; out[i] = g[0]*scale (its backward) */
int pg_vec_mean_accum(const float* v, int n, float* out, void* stream);
int pg_fill_scaled(const float* g, float scale, float* out, int n, void* stream);

/* ---------------------------------------------------------------------------------------
 * The transformer block's position-wise MLP, fused.  models/autoregressive/image_gpt.py:43-52:
 *   y = res + W2 gelu(W1 x + b1) + b2     (Conv2d(C,Hd,1) -> GELU -> Conv2d(Hd,C,1), `x + self._out(..)`)
 * x, res, y, dy, dx: (N, C, L); w1: (Hd, C); w2: (C, Hd); exact (erf) GELU. The hidden tensor is
 * never written to memory; backward recomputes it. Instantiated for C = 16, Hd = 64, L % 16 == 0
 * (PG_ESHAPE otherwise: the caller runs the three unfused operators). res may be NULL.
 * Backward: dx is written; dw1/db1/dw2/db2 are ADDED to (per-workgroup partial rows in `workspace`,
 * then a deterministic reduce); d(res) = dy is the caller's. x and dy must be 16-byte aligned.
 * ------------------------------------------------------------------------------------- */
int pg_mlp_gelu_fwd(const float* x, const float* w1, const float* b1, const float* w2,
                    const float* b2, const float* res, float* y, int N, int C, int Hd, int L,
                    void* stream);
int pg_mlp_gelu_bwd(const float* x, const float* w1, const float* b1, const float* w2,
                    const float* dy, float* dx, float* dw1, float* db1, float* dw2, float* db2,
                    int N, int C, int Hd, int L, float* workspace, size_t workspace_floats,
                    void* stream);
size_t pg_mlp_gelu_bwd_workspace_floats(int N, int L);

/* ---------------------------------------------------------------------------------------
 * Everything of an ImageGPT transformer block except the attention core, fused (gpt_block.hip).
 * models/autoregressive/image_gpt.py:21-52 and the model loop :104-109, C = 16, hidden Hd = 64:
 *   head: qkv (N,48,L) = [W_q; W_kv] LN1(x) + [b_q; b_kv]       (_ln1, _attn._q, _attn._kv)
 *   tail: x_mid = x + W_p o + b_p ; x_new = x + x_mid + W_2 gelu(W_1 LN2(x_mid) + b_1) + b_2
 *         (_attn._proj + residual, _ln2, _out, residual, and the model loop's `x = x + block(x)`)
 * Backward recomputes x_mid, the LayerNorms and the hidden activations from (x, o).
 *   tail_bwd: dx_new -> d_o (gradient of the attention output) and gx (all of dx_new that reaches x
 *             except through LN1); head_bwd: dx = LN1'(W^T dqkv) + gx.
 * Parameter gradients are ADDED to (partial rows in `workspace` + deterministic reduce).
 * Instantiated for C = 16, Hd = 64, L % 16 == 0 (PG_ESHAPE otherwise: run the unfused operators).
 * dqkv, o and dx_new must be 16-byte aligned.
 * ------------------------------------------------------------------------------------- */
int pg_gpt_block_head_fwd(const float* x, const float* ln_w, const float* ln_b, const float* wq,
                          const float* bq, const float* wkv, const float* bkv, float* qkv, int N,
                          int C, int L, float eps, void* stream);
int pg_gpt_block_head_bwd(const float* x, const float* ln_w, const float* ln_b, const float* wq,
                          const float* wkv, const float* dqkv, const float* gx, float* dx,
                          float* dln_w, float* dln_b, float* dwq, float* dbq, float* dwkv,
                          float* dbkv, int N, int C, int L, float eps, float* workspace,
                          size_t workspace_floats, void* stream);
size_t pg_gpt_block_head_bwd_workspace_floats(int N, int L);
int pg_gpt_block_tail_fwd(const float* o, const float* x, const float* wp, const float* bp,
                          const float* ln_w, const float* ln_b, const float* w1, const float* b1,
                          const float* w2, const float* b2, float* x_new, int N, int C, int Hd,
                          int L, float eps, void* stream);
int pg_gpt_block_tail_bwd(const float* o, const float* x, const float* wp, const float* bp,
                          const float* ln_w, const float* ln_b, const float* w1, const float* b1,
                          const float* w2, const float* dx_new, float* d_o, float* gx, float* dwp,
                          float* dbp, float* dln_w, float* dln_b, float* dw1, float* db1,
                          float* dw2, float* db2, int N, int C, int Hd, int L, float eps,
                          float* workspace, size_t workspace_floats, void* stream);
size_t pg_gpt_block_tail_bwd_workspace_floats(int N, int L);
/* A block boundary of the forward pass in ONE launch: the tail of block i (image_gpt.py:21-52 and the model loop's
 * `x = x + block(x)`, :104-109) and the head of block i+1 (its _ln1, _attn._q, _attn._kv) on the x_new tile while it is
 * still in registers. Replaces pg_gpt_block_tail_fwd(..., x_new) followed by pg_gpt_block_head_fwd(x_new, next_*, next_qkv)
 * and writes the same bits to both outputs (the same device functions; x_new is written but not read back). The first
 * eleven pointers and N, C, Hd, L are pg_gpt_block_tail_fwd's; next_* are pg_gpt_block_head_fwd's parameters of the
 * following block. eps is used by both LayerNorms. PG_ESHAPE under the conditions of the two launchers it replaces. */
int pg_gpt_block_tail_head_fwd(const float* o, const float* x, const float* wp, const float* bp,
                               const float* ln_w, const float* ln_b, const float* w1, const float* b1,
                               const float* w2, const float* b2, float* x_new, const float* next_ln_w,
                               const float* next_ln_b, const float* next_wq, const float* next_bq,
                               const float* next_wkv, const float* next_bkv, float* next_qkv, int N, int C,
                               int Hd, int L, float eps, void* stream);
/* The two backward kernels WITHOUT their reductions: each leaves its rows of partial weight-gradient sums in `workspace`
 * (pg_gpt_block_*_bwd_workspace_floats floats; keep it alive) and touches no gradient. pg_gpt_model_reduce, declared with
 * ImageGPT's ends below, adds the rows of up to 8 blocks to their gradients in one launch. The gradients are bit for bit those of
 * pg_gpt_block_tail_bwd + pg_gpt_block_head_bwd, however the blocks are grouped into launches: the same kernel adds every
 * column's rows in the same order. */
int pg_gpt_block_tail_bwd_partial(const float* o, const float* x, const float* wp, const float* bp,
                                  const float* ln_w, const float* ln_b, const float* w1, const float* b1,
                                  const float* w2, const float* dx_new, float* d_o, float* gx, int N, int Cc,
                                  int Hd, int L, float eps, float* workspace, size_t workspace_floats,
                                  void* stream);
int pg_gpt_block_head_bwd_partial(const float* x, const float* ln_w, const float* ln_b, const float* wq, const float* wkv,
                                  const float* dqkv, const float* gx, float* dx, int N, int C, int L, float eps,
                                  float* workspace, size_t workspace_floats, void* stream);
/* A block boundary of the backward pass in ONE launch: pg_gpt_block_head_bwd_partial of block i+1 (next_*: its x, parameters,
 * dqkv and gx) and pg_gpt_block_tail_bwd_partial of block i (the rest) on the head's dx tile while it is still in registers; dx
 * itself, the tail's dx_new, is not written anywhere. d_o and gx hold the same bits as after the two launches. head_workspace and
 * tail_workspace (pg_gpt_block_head_bwd_workspace_floats / pg_gpt_block_tail_bwd_workspace_floats floats) receive the partial rows
 * of block i+1's head job and block i's tail job for pg_gpt_model_reduce: one row per workgroup of this launch and zeros in the
 * rest, so the parameter gradients equal those of the two launches up to the order of the sums. eps is used by both LayerNorms. */
int pg_gpt_block_head_tail_bwd_partial(const float* next_x, const float* next_ln_w, const float* next_ln_b,
                                       const float* next_wq, const float* next_wkv, const float* next_dqkv,
                                       const float* next_gx, const float* o, const float* x, const float* wp, const float* bp,
                                       const float* ln_w, const float* ln_b, const float* w1, const float* b1, const float* w2,
                                       float* d_o, float* gx, int N, int C, int Hd, int L, float eps, float* head_workspace,
                                       size_t head_workspace_floats, float* tail_workspace, size_t tail_workspace_floats,
                                       void* stream);

/* ---------------------------------------------------------------------------------------
 * Incremental autoregressive sampling (models/base.py:97-120 runs H*W full forwards; the causal
 * models need only position p per step). Activations of one position live as (channels, ld) matrices,
 * column n = sample n, so the block kernels above apply with N = 1, L = ld.
 *   pg_sample_embed: out[co*ld + n] = pixel (r, c) of Conv2d(w (already masked), b, padding k/2)
 *                    applied to canvas (N,Cin,H,W) + pos (Cin,H,W or NULL)   (image_gpt.py:105)
 *   pg_attn_decode:  qkv = rows [q (heads*dk) | k (heads*dk) | v (heads*dv)] x ld; appends k, v to
 *                    the caches (N, heads*dk, L) / (N, heads*dv, L) at column p and writes
 *                    o (heads*dv rows x ld) = softmax over positions <= p - strict   (attention.py:147-160)
 * pos_dev (device int, or NULL): when given, the raster position p (and r = p / W, c = p % W) is read
 * from it instead of the host arguments, so that one captured hipGraph can be replayed per pixel.
 * ------------------------------------------------------------------------------------- */
int pg_sample_embed(const float* canvas, const float* pos, const float* w, const float* b, float* out,
                    int N, int Cin, int H, int W, int Cout, int KH, int KW, int r, int c, int ld,
                    const int* pos_dev, void* stream);
int pg_attn_decode(const float* qkv, float* k_cache, float* v_cache, float* o, int N, int heads,
                   int L, int p, int dk, int dv, int ld, int strict, const int* pos_dev,
                   void* stream);

/* ---------------------------------------------------------------------------------------
 * One raster position of ALL transformer blocks of ImageGPT in one launch (csrc/gpt_decode.hip): one workgroup per
 * sample, activations in LDS, any width. x and out: (C, ld) planes, column n = sample n, as pg_sample_embed writes them;
 * out may be x. Per block, on one column (image_gpt.py:50-52 with :107-108):
 *   a = LN1(h); [q | k | v] = Wqkv a + b; caches[:, p] = k, v; o = softmax_{j <= p - strict}(q . k_j / sqrt(dk)) v_j per
 *   head (0 when no key is admitted); b = h + Wproj o + bproj; m = W2 gelu(W1 LN2(b) + b1) + b2 (erf GELU); h = h + (b + m).
 * k_cache, v_cache: (blocks, N, C, L). The launch writes cache column p of every block and no other cache entry, and reads
 * none beyond p. p from the host, or *pos_dev (device int, or NULL) clamped to [0, L - 1] as pg_attn_decode does.
 * pack: the parameters of all blocks in one float buffer, block i at i * block_floats, inside a block the PG_GD_* fields
 * at the offsets the plan reports; every weight matrix is stored TRANSPOSED, (in, out) row-major:
 *   LN1_W, LN1_B (C) | WQKV (C, 3C) = [_q ; _kv] weights transposed, BQKV (3C) | WPROJ (C, C), BPROJ (C) |
 *   LN2_W, LN2_B (C) | W1 (C, 4C), B1 (4C) | W2 (4C, C), B2 (C)
 * No float atomics, every reduction in a fixed order: column n of out is bit-identical from run to run and for any N, ld.
 * pg_gpt_decode_plan (host only, no device call) is the one function that decides the domain; the launch calls it too.
 * It fills out[0 .. PG_GPT_DECODE_PLAN_INTS): pack floats, floats per block, LDS bytes per workgroup (at most 64 KB),
 * threads per workgroup, then the PG_GPT_DECODE_FIELDS field offsets. C a multiple of 4 in 4..256, heads dividing C,
 * blocks in 1..64, L in 1..4096 (PG_ESHAPE otherwise, from the plan and the launch alike, nothing launched); PG_EINVAL for
 * a null pointer, a short array, a non-positive dimension, ld < N, strict not 0/1 or a host p outside [0, L).
 * ------------------------------------------------------------------------------------- */
enum {
  PG_GD_LN1_W = 0, PG_GD_LN1_B, PG_GD_WQKV, PG_GD_BQKV, PG_GD_WPROJ, PG_GD_BPROJ,
  PG_GD_LN2_W, PG_GD_LN2_B, PG_GD_W1, PG_GD_B1, PG_GD_W2, PG_GD_B2
};
#define PG_GPT_DECODE_FIELDS 12
#define PG_GPT_DECODE_PLAN_INTS 16
int pg_gpt_decode_plan(int C, int heads, int blocks, int L, int* out, int out_len);
int pg_gpt_decode_step(const float* x, float* out, const float* pack, float* k_cache, float* v_cache, int N, int C,
                       int heads, int blocks, int L, int ld, int p, int strict, float eps, const int* pos_dev,
                       void* stream);

/* ---------------------------------------------------------------------------------------
 * Row-cached sampling of the convolutional models with attention (PixelSNAIL; csrc/attention_row.hip): the W queries of
 * image row r against K / V caches of the rows above, one launch of a static shape. All tensors contiguous fp32, dk / dv
 * per head, head h owning the channel block [h*d, (h+1)*d) (reference nn/attention.py, _to_multihead):
 *   q_row (N, heads*dk, 1, W); kv_row (N, heads*dk + heads*dv, 1, W), keys first; k_cache (N, heads*dk, H, W);
 *   v_cache (N, heads*dv, H, W); o_row (N, heads*dv, 1, W).
 * Query column x of row r admits every cache key of rows y < r, the keys x' < x of row r, and x' == x when mask_center is 0;
 * the keys and values of row r itself come from kv_row, never from the cache.
 *   o = sum_j softmax_j(q . k_j / sqrt(dk)) v_j over the admitted set; exactly 0 when nothing is admitted.
 * write_cache = 1: the launch also stores kv_row's k and v, bit for bit, into cache row r. It reads no cache row >= r and
 * writes no row other than r. r from the host, or *row_dev (device int, or NULL) clamped to [0, H - 1], the host r then
 * being ignored, as pg_attn_decode treats pos_dev: one captured hipGraph replays for every row.
 * No float atomics, every reduction in a fixed order: sample n's output is bit-identical from run to run and for any N.
 * pg_attn_row_plan (host only, no device call) is the one function that decides the domain and the launch geometry; the
 * launch calls it too. It fills out[0 .. PG_ATTN_ROW_PLAN_INTS): threads per workgroup, LDS bytes per workgroup, keys per
 * LDS tile, grid x (workgroups per row), grid y (heads; grid z is N), queries per workgroup. heads >= 1, dk in 1..64,
 * dv in 1..128, W in 1..256, H*W <= 4096 (PG_ESHAPE otherwise, from the plan and the launch alike, and from the launch for
 * N above 65535; nothing launched); PG_EINVAL for a null pointer, a short array, a non-positive dimension, a host r outside
 * [0, H) or a flag that is not 0/1.
 *   pg_row_gather: dst (N, C, 1, W) = src (N, C, H, W)[:, :, r], r as above (the positional-encoding row of the step).
 * ------------------------------------------------------------------------------------- */
#define PG_ATTN_ROW_PLAN_INTS 6
int pg_attn_row_plan(int heads, int dk, int dv, int H, int W, int* out, int out_len);
int pg_attn_row(const float* q_row, const float* kv_row, float* k_cache, float* v_cache, float* o_row, int N, int heads,
                int dk, int dv, int H, int W, int r, int mask_center, int write_cache, const int* row_dev, void* stream);
int pg_row_gather(const float* src, float* dst, int N, int C, int H, int W, int r, const int* row_dev, void* stream);

/* ---------------------------------------------------------------------------------------
 * Optimiser step as timed by the reference (trainer.py:183-191): global grad L2 norm
 * (clip_grad_norm_) + torch.optim.Adam over ONE flat parameter/grad buffer.
 * state (device, 8 floats): [0]=step count, [1]=lr, [2]=sum of squares (scratch),
 *   [3]=grad norm (output), [4]=clip coefficient (output), [5]=lr multiplier per step,
 *   [6]=max_norm, [7]=grad pre-scale (1/world after all-reduce)
 * ------------------------------------------------------------------------------------- */
int pg_sumsq_accum(const float* g, size_t n, float* state, void* stream);
int pg_adam_prepare(float* state, void* stream);
/* The same two steps with a run-to-run reproducible norm (what FlatAdam launches): the norm kernel's
 * blocks store their partial sums to partials[0 .. pg_sumsq_partial_count(n)) (at most 1024 floats, no
 * atomics, nothing to zero) and the prepare kernel adds them in a fixed order. state[2] is not used.
 * nparts MUST be pg_sumsq_partial_count(n) of the n just given to pg_sumsq_partials: entries beyond it
 * were not written by that launch. */
int pg_sumsq_partial_count(size_t n);
int pg_sumsq_partials(const float* g, size_t n, float* partials, void* stream);
int pg_adam_prepare_ordered(float* state, const float* partials, int nparts, void* stream);
int pg_adam_step(float* p, const float* g, float* m, float* v, size_t n, const float* state,
                 float beta1, float beta2, float eps, void* stream);

/* ---------------------------------------------------------------------------------------
 * SURVEY.md §8(f) rank 4 — vector quantisation (reference nn/utils.py:53-96) and the MSE loss of
 * the VQ-VAE recipes (models/vae/vq_vae.py:127-136). csrc/vq.hip; reached through
 * pytorch_generative_amd/nn/utils.py (VectorQuantizer, mse_loss). Validated on MI355X against outputs
 * of the reference (tests/test_gpu_f4.py).
 * ------------------------------------------------------------------------------------- */
/* x (N, D, L) NCHW planes, embedding (K, D), D <= 64. Per position p = n*L + l: idx[p] = first
 * argmin_k (|x|^2 + |e_k|^2) - 2 x.e_k (nn/utils.py:61-68); q = embedding[idx] in NCHW;
 * st = x + (q - x) (the straight-through VALUE, :95); loss[0] += mean((x - q)^2) (:79; zeroed by caller) */
int pg_vq_assign(const float* x, const float* embedding, int* idx, float* q, float* st, float* loss,
                 int N, int D, int L, int K, void* stream);
/* EMA codebook update in place (nn/utils.py:80-90): count / sum of x per code (workspaces count_ws
 * (K), sum_ws (K*D), zeroed inside), cluster_size = cluster_size*decay + count*(1-decay), the same
 * for embedding_avg, embedding = embedding_avg / (cluster_size + 1e-5) */
int pg_vq_ema_update(const float* x, const int* idx, float* cluster_size, float* embedding_avg,
                     float* embedding, float* count_ws, float* sum_ws, int N, int D, int L, int K,
                     float decay, void* stream);
/* dx = d_st + g_loss[0] * 2 (x - q) / n  (straight-through + commitment loss) */
int pg_vq_bwd(const float* x, const float* q, const float* d_st, const float* g_loss, float* dx,
              size_t n, void* stream);
/* pg_vq_assign for any D >= 1 (csrc/vq_mfma.hip): the distances as a tiled fp32-MFMA GEMM with a running
 * (best, index) per position, codes visited in ascending order with a strict '<' (first minimum). Same
 * operands and outputs as pg_vq_assign. PG_ESHAPE for a non-positive dimension, D > 2^20, K > 65535 * 64,
 * N * L > 2^31 - 65 or K * D >= 2^31; PG_EINVAL for a null operand. */
int pg_vq_assign_tiled(const float* x, const float* embedding, int* idx, float* q, float* st, float* loss,
                       int N, int D, int L, int K, void* stream);
/* Gradient of the embedding loss mse(q, x.detach()) of a codebook trained by gradient descent (nn/utils.py:93):
 *   d_embedding[k][d] (+)= g_loss[0] * (2 / (N L D)) * sum_{p : idx[p] = k} (q[p][d] - x[p][d])
 * as onehot(idx)^T (q - x) over ranges of positions into `ws` (pg_vq_codebook_grad_workspace_floats floats; every word
 * that is read is written first), merged in range order: no float atomics, bit-reproducible. accumulate != 0 adds
 * into d_embedding (a flat-gradient sink). Shape errors as pg_vq_assign_tiled; PG_EINVAL for a null operand or a
 * short workspace. The query returns 0 for shapes the launch refuses. */
size_t pg_vq_codebook_grad_workspace_floats(int N, int D, int L, int K);
int pg_vq_codebook_grad(const float* x, const float* q, const int* idx, const float* g_loss, float* d_embedding,
                        int accumulate, int N, int D, int L, int K, float* ws, size_t ws_floats, void* stream);
/* loss[0] += mean((a - b)^2) (zeroed by caller); da = g_loss[0] * 2 (a - b) / n, db = -da
 * (either may be NULL) */
int pg_mse_fwd(const float* a, const float* b, float* loss, size_t n, void* stream);
int pg_mse_bwd(const float* a, const float* b, const float* g_loss, float* da, float* db, size_t n,
               void* stream);

/* PixelCNN++'s concatenated ELU (Salimans et al. 2017, section 2.3; not in the reference):
 * y (N, 2C, L) = [elu(x) | elu(-x)]; CL = C * L. */
int pg_concat_elu_fwd(const float* x, float* y, int N, long CL, void* stream);
int pg_concat_elu_bwd(const float* x, const float* dy, float* dx, int N, long CL, void* stream);

/* Discretized mixture-of-logistics negative log-likelihood (the PixelCNN++ loss of BASELINE.json
 * configs[2]; absent from the reference: Salimans et al., ICLR 2017, eq. (2)-(3), restated in
 * oracle/dmol.py). l (N, 10 K, L): K logits, then per sub-pixel c = 0..2: K means, K log-scales, K raw
 * coefficients; x (N, 3, L) in [-1, 1]; K <= 16.
 *   fwd: loss[0] += -(1 / N) sum log p(x) (nats; zeroed by the caller)
 *   bwd: dl = gscale[0] * d loss / d l */
int pg_dmol_fwd(const float* l, const float* x, float* loss, int N, int K, int L, void* stream);
int pg_dmol_bwd(const float* l, const float* x, const float* gscale, float* dl, int N, int K, int L,
                void* stream);

/* One pixel's draw from the logistic mixture for all N images, in ONE launch (the per-pixel step of PixelCNN++'s row-cached
 * sampler; the arithmetic of PixelCNNpp.sample_from_mixture followed by where(unknown, drawn, canvas)):
 *   component = argmax_k (logit_k - log(-log u_k)), u clamped to [1e-5, 1 - 1e-5]; per sub-pixel a logistic variate
 *   mean + exp(max(log_scale, -7)) * (log v - log1p(-v)); G and B shifted by tanh(coefficient) times the DRAWN R / G (also
 *   where a given value is kept); each clamped to [-1, 1].
 * params: the row's (N, 10 K, 1, W) parameters in the channel layout of pg_dmol_fwd, read at column c through its strides
 * sp_n / sp_c / sp_w (in floats); uniforms (H * W, N, K + 3): K for the component, 3 for the sub-pixels, read at raster
 * position p = r * W + c; canvas (N, 3, H, W) and its byte mask `unknown` (non-zero = draw): canvas[n, :, r, c] is
 * replaced where unknown; row_buf (N, 3, 1, W) or NULL: receives canvas[n, :, r, c] as it stands after the draw.
 * pos_dev (device int, or NULL): the raster position, as for pg_sample_embed (clamped to the image; r, c are then ignored
 * but must still be valid). Any N >= 1; H, W multiples of 4; 1 <= K <= PG_DMOL_SAMPLE_MAX_K (PG_ESHAPE otherwise);
 * PG_EINVAL for a null operand, a non-positive stride or a pixel outside the image. No device call before these checks. */
#define PG_DMOL_SAMPLE_MAX_K 32
int pg_dmol_sample(const float* params, long sp_n, long sp_c, long sp_w, const float* uniforms, float* canvas,
                   const unsigned char* unknown, float* row_buf, int N, int K, int H, int W, int r, int c,
                   const int* pos_dev, void* stream);

/* Column resampling of `rows` dense rows (the strided levels of PixelCNN++ on ONE image row):
 *   pg_col_subsample2:   y[row][q] = x[row][2 q], x rows of W floats (W even), y rows of W / 2
 *   pg_col_zero_insert2: y[row][2 q] = x[row][q], y[row][2 q + 1] = 0, x rows of W floats, y rows of 2 W
 * PG_ESHAPE for rows <= 0, W <= 0 or an odd W to sub-sample; PG_EINVAL for a null operand. */
int pg_col_subsample2(const float* x, float* y, long rows, int W, void* stream);
int pg_col_zero_insert2(const float* x, float* y, long rows, int W, void* stream);

/* dst[r * dst_stride + i] (+)= src[r * src_stride + i] for r < rows, i < row_len (strides in floats).
 * The channel concatenation in front of a merged projection (nn/attention.py:139-143
 * torch.cat((x, extra_x), dim=1): a row = the channels of one image) and the assembly / gradient split
 * of that projection's merged weight. accumulate != 0 adds into dst. */
int pg_copy_rows(const float* src, float* dst, long rows, long row_len, long src_stride,
                 long dst_stride, int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------
 * Data-parallel exchange step: replaces DistributedDataParallel's gradient
 * all-reduce (reference trainer.py:78-82; process group of train.py:27-37) by ONE RCCL all-reduce of
 * the flat gradient buffer over xGMI. csrc/comm.hip binds librccl at run time (the copy the process
 * already carries, if any). One communicator per process (= per GPU).
 *   rank 0: pg_comm_unique_id(id) -> ship the 128 bytes to every rank out of band (the host side uses
 *   the torch.distributed rendezvous for that and for nothing else) -> every rank: pg_comm_init.
 * pg_allreduce_sum / pg_broadcast are in place, asynchronous, enqueue only on `stream`, do not
 * allocate or synchronise: they may be captured inside the hipGraph of the training step.
 * Return values: 0, PG_E*, or 1000 + ncclResult_t.
 * ------------------------------------------------------------------------------------- */
#define PG_COMM_ID_BYTES 128
#define PG_DTYPE_F32 0
int pg_comm_unique_id(char id[PG_COMM_ID_BYTES]);
int pg_comm_init(int rank, int world, const char id[PG_COMM_ID_BYTES]); /* on the current device */
int pg_comm_world(void);        /* world size of the live communicator, 0 if none */
int pg_comm_rccl_version(void); /* ncclGetVersion of the bound library, 0 if it cannot be bound */
int pg_allreduce_sum(void* buf, size_t n, int dtype, void* stream);
int pg_broadcast(void* buf, size_t n, int dtype, int root, void* stream);
int pg_comm_destroy(void);

/* ---------------------------------------------------------------------------------------
 * ImageGPT's two ends (models/autoregressive/image_gpt.py: the first and the last line of forward), gpt_ends.hip.
 * fp32; C = 16 embedding channels; 1 <= Cout <= 4. grid_cap: upper bound on the workgroups of the launch, 0 = the
 * library's default (persistent workgroups walk the tiles). Reductions are deterministic: the backward kernels leave
 * partial rows in `workspace`, pg_gpt_model_reduce adds them (to what the destinations hold).
 *
 * stem: x0 (N,16,H*W) = CausalConv2d type A 3x3, padding 1, of img (N,1,H,W) + pos (1,1,H,W); zero padding applies to the
 * sum. The forward also zeroes the masked entries of `weight` (16,1,3,3) in place (taps 4..8 of every output channel), which
 * it never reads. The backward leaves d weight for all nine taps, d bias and the position-wise sums d pos is gathered from;
 * its workspace holds pg_gpt_stem_bwd_workspace_floats floats, laid out for the rows / slices of pg_gpt_stem_bwd_plan.
 * head: logits (N,Cout,L) = Conv1x1(LayerNorm over channels of x (N,16,L)), LayerNorm as in the block kernels (biased
 * variance, eps inside the root). The backward writes dx and pg_gpt_out_head_bwd_rows rows of 32 + 17 Cout floats. */
int pg_gpt_stem_fwd(const float* img, const float* pos, float* weight, const float* bias, float* x0, int N, int H, int W,
                    int grid_cap, void* stream);
int pg_gpt_stem_bwd_plan(int N, int H, int W, int grid_cap, int* rows, int* slices);
size_t pg_gpt_stem_bwd_workspace_floats(int N, int H, int W, int grid_cap);
int pg_gpt_stem_bwd(const float* dx0, const float* img, const float* pos, const float* weight, int N, int H, int W,
                    int grid_cap, float* workspace, size_t workspace_floats, void* stream);
int pg_gpt_out_head_fwd(const float* x, const float* ln_w, const float* ln_b, const float* conv_w, const float* conv_b,
                        float* logits, int N, int C, int Cout, int L, float eps, int grid_cap, void* stream);
int pg_gpt_out_head_bwd_rows(int N, int L, int grid_cap);
int pg_gpt_out_head_bwd(const float* x, const float* ln_w, const float* ln_b, const float* conv_w, const float* dlogits,
                        float* dx, int N, int C, int Cout, int L, float eps, int grid_cap, float* workspace,
                        size_t workspace_floats, void* stream);
/* ONE launch that adds partial rows to gradients: those of n_blocks (0..8) transformer blocks, as left by
 * pg_gpt_block_head_bwd_partial (head_ws[b]) and pg_gpt_block_tail_bwd_partial (tail_ws[b]) for the same N, C, L, and those of
 * either end. head_ws, tail_ws, grads, out_grads and stem_grads are HOST arrays of device pointers. grads: n_blocks x 14, per block
 * dln1_w, dln1_b, dwq, dbq, dwkv, dbkv, then the tail's dw1, db1, dw2, db2, dwp, dbp, dln2_w, dln2_b. out_ws / stem_ws may be
 * null (that end is left out; with n_blocks = 0 at least one must be given). out_grads: d ln.weight, d ln.bias, d conv.weight,
 * d conv.bias; stem_grads: d weight, d bias, d pos. Everything is added to what the destinations hold. */
int pg_gpt_model_reduce(int n_blocks, const float* const* head_ws, const float* const* tail_ws, float* const* grads, int N,
                        int C, int L, const float* out_ws, int out_rows, int Cout, float* const* out_grads,
                        const float* stem_ws, int stem_rows, int stem_slices, int H, int W, float* const* stem_grads,
                        void* stream);

/* ---------------------------------------------------------------------------------------
 * Categorical (K-way softmax) pixel likelihood, categorical.hip: the likelihood PixelCNN, GatedPixelCNN, PixelSNAIL and
 * ImageGPT were published with. logits (N, K C, H, W) dense, read as (N, K, C, HW): class-major, the layout
 * F.cross_entropy takes as logits.view(N, K, C, H, W). x: images (N, C, HW) at the levels j / (K - 1); the class of a
 * sub-pixel is t = clamp((int)rintf(x (K - 1)), 0, K - 1).
 *   fwd:    lse (2, N, C, HW): plane 0 is lse[n, c, p] = logsumexp_k z as max + log(sum exp(z - max)), plane 1 the fp32
 *           rounding residual of that last addition (the backward needs the normaliser to better than one ulp of a large
 *           lse); loss[0] += (1 / N) sum (lse - z_t) (nats; zeroed by the caller; fp32 atomics in arrival order, as
 *           pg_bce_logits_fwd); per_sample (N) or NULL: sum over the image's sub-pixels of lse - z_t, in a fixed order.
 *   bwd:    dlogits = g[0] / N * (exp(z - lse) - [k == t]) from the forward's two planes; no reduction: bit-reproducible.
 *   sample: one position's draw. logits (N, K C) with element strides (sn, sk): the logit of (n, k, c) is at
 *           n * sn + (k * C + c) * sk; uniforms (N, C) in [0, 1); out (N, C). With e_k = exp((z_k - max_k z) *
 *           inv_temperature): the first class whose inclusive running sum exceeds u * sum_k e_k strictly, the last class
 *           if rounding leaves none; out = class / (K - 1).
 *   plan:   host only, no device needed: the lanes that share one sub-pixel's classes (K / 64 rounded down to a power
 *           of two, 1..8; N, C and HW do not change it) and the sub-pixels per lane (4 when HW % 4 == 0, else 1) of the
 *           fwd / bwd launches with 16-byte aligned operands (others take vec = 1).
 * K in 2..4096, N, C, HW >= 1, N * C * HW < 2^31, N * C * HW * K < 2^40 (PG_ESHAPE otherwise); PG_EINVAL for a null
 * operand (per_sample excepted), a non-positive stride or inverse temperature. No device call before these checks. */
int pg_categorical_plan(int N, int C, int K, int HW, int* lanes_per_pixel, int* vec);
int pg_categorical_nll_fwd(const float* logits, const float* x, float* lse, float* per_sample, float* loss, int N, int C,
                           int K, int HW, void* stream);
int pg_categorical_nll_bwd(const float* logits, const float* x, const float* lse, const float* g, float* dlogits, int N,
                           int C, int K, int HW, void* stream);
int pg_categorical_sample(const float* logits, long sn, long sk, const float* uniforms, float* out, int N, int C, int K,
                          float inv_temperature, void* stream);

/* ---------------------------------------------------------------------------------------
 * The last 1x1 convolution fused into the categorical likelihood, linear_categorical.hip:
 *   loss = categorical_nll(conv1x1(transform(h))) with nothing of the logits' size N K C HW written in either pass.
 * h (N, Cin, HW) dense; w (K C, Cin) the convolution's weight, class-major (output channel k C + c), 16-byte aligned;
 * b (K C) or NULL; x as above. transform (PG_LC_*) is applied to h on load: none, relu, or LayerNorm over the Cin
 * channels with (ln_w, ln_b, eps) (biased variance, eps inside the root; both 16-byte aligned, NULL otherwise).
 *   plan:   host only. A workgroup (one wave) owns ceil(tiles / rows) consecutive tiles of `pixels_per_tile` consecutive
 *           pixels of the sequence n HW + hw; `rows` workgroups = partial rows; `lds_bytes` the largest LDS a launch takes;
 *           workspace_floats = rows * (K C Cin + K C + 2 Cin). rows * row length stays within a quarter of N K C HW
 *           floats unless a single row exceeds that (rows = 1 then).
 *   fwd:    lse (2, N, C, HW) as pg_categorical_nll_fwd — (3, N, C, HW) when per_sample is given: plane 2 then receives the
 *           sub-pixel's lse - z_t, which per_sample (N) sums in a fixed order; loss[0] += (1 / N) sum (lse - z_t), one fp32
 *           atomic per workgroup.
 *   bwd:    recomputes the logits bit for bit, d = g[0] / N (exp((z - lse) - residual) - [k == t]); writes
 *           dh (N, Cin, HW) (through the transform's derivative) and one partial row per workgroup into `workspace`:
 *           [ dW (K C x Cin) | db (K C) | d ln_w (Cin) | d ln_b (Cin) ] (parts that do not apply stay zero).
 *           Where |lse| of a sub-pixel is 16 or more (8 for Cin > 64) the classes within 18 of it are evaluated once more in
 *           float64, in both passes: lse + residual is the normaliser of the exact logits to 4e-6, whatever their size.
 *   reduce: ADDS the rows, in row order, into dW and (where not NULL) db, dln_w, dln_b. No float atomics on a gradient.
 * Cin a multiple of 4 in 4..256, K in 2..4096, the size limits of pg_categorical_*, N HW < 2^31 - 16 and
 * K C (Cin + 1) + 2 Cin < 2^31 (PG_ESHAPE otherwise); PG_EINVAL for a null or misaligned operand or a short workspace.
 * No device call before these checks. */
#define PG_LC_NONE 0
#define PG_LC_RELU 1
#define PG_LC_LN 2
int pg_linear_categorical_plan(int N, int C, int K, int Cin, int HW, int transform, int* pixels_per_tile, int* rows,
                               int* lds_bytes, size_t* workspace_floats);
int pg_linear_categorical_nll_fwd(const float* h, const float* w, const float* b, const float* ln_w, const float* ln_b,
                                  float eps, const float* x, float* lse, float* per_sample, float* loss, int N, int C, int K,
                                  int Cin, int HW, int transform, void* stream);
int pg_linear_categorical_nll_bwd(const float* h, const float* w, const float* b, const float* ln_w, const float* ln_b,
                                  float eps, const float* x, const float* lse, const float* g, float* dh, int N, int C, int K,
                                  int Cin, int HW, int transform, float* workspace, size_t workspace_floats, void* stream);
int pg_linear_categorical_reduce(const float* workspace, int rows, int KC, int Cin, int transform, float* dW, float* db,
                                 float* dln_w, float* dln_b, void* stream);

/* ---------------------------------------------------------------------------------------
 * Convolution over an image of code indices, code_conv.hip: F.conv2d(one_hot(codes), w) as a table lookup, for
 * autoregressive priors over VQ-VAE codes. levels (N, 1, Hin, Win) dense: a code image at the levels j / (K - 1) (the
 * layout pg_categorical_nll_* take as x; the code is clamp((int)rintf(level (K - 1)), 0, K - 1)); a NEGATIVE level is an
 * undrawn position and stands for the all-zero one-hot vector. w (Cout, K, KH, KW).
 *   fwd:    out[n, :, y, x] = b + sum_t w[:, code(n, y + u_t - pad_h, x + v_t - pad_w), u_t, v_t] over the tap list
 *           (u, v) (host arrays; inside the kernel, strictly ascending in u KW + v), zero outside the image;
 *           out (N, Cout, OH, OW) is any window anchored at the top-left corner (a row band is the same call with another
 *           pad_h). The taps are packed once per call into a (taps, K, Cout) table in `ws`
 *           (pg_code_conv_fwd_workspace_floats floats). Bias first, then the taps in ascending order: bit-reproducible.
 *           b may be NULL. The caller has masked w already.
 *   wgrad:  dw[co, k, u, v] (+)= sum of dy[n, co, y, x] over the positions with code(n, y + u - pad_h, x + v - pad_w) = k,
 *           for ALL KH KW taps (the reference's weight gradient is unmasked), db[co] (+)= sum dy[:, co]; either may be
 *           NULL. Store-and-sum: an inverted index (per code the ascending list of its positions: a stable counting sort
 *           on integer counters), one wave sums a chunk of at most 512 list entries for a group of channels, a code's
 *           chunks are added in chunk order. No float atomics, no host synchronisation, capturable; bit-reproducible.
 *           Codes that never occur receive exact zeros. accumulate != 0 adds the finished sum to dw / db (a flat-gradient
 *           sink) with one fp32 addition per element. ws: pg_code_conv_wgrad_workspace_floats floats (every word that is
 *           read is written first).
 *   plan:   host only. max_chunks = the chunks of the longest possible list, ceil(N Hin Win / 512); items = the work
 *           items reserved for the sum, K + N Hin Win / 512 (an upper bound of sum_k ceil(list_k / 512)).
 * pg_sample_embed_codes: the code counterpart of pg_sample_embed. out[co * ld + n] = b[co] + pos_term[co, r, c] + the
 *   stem at raster position (r, c) of every sample (pos_dev != NULL: the position is read from the device), padding
 *   KH / 2, KW / 2, every tap read (w is masked). canvas (N, 1, H, W) levels, pos_term (Cout, H, W) or NULL.
 * pg_vq_lookup: out (N, D, L) = embedding[code(levels (N, L))] transposed: the VQ-VAE decoder's input from a code image
 *   (a negative level reads code 0).
 * K in 2..4096, at most PG_MAX_TAPS taps, positions and weights below 2^31 (PG_ESHAPE otherwise); PG_EINVAL for a null
 * operand, a bad tap list, a pixel outside the image or a short workspace. No device call before these checks; the queries return 0 for shapes
 * the launch refuses. */
size_t pg_code_conv_fwd_workspace_floats(int Cout, int K, int n_taps);
int pg_code_conv_fwd(const float* levels, const float* w, const float* b, float* out, int N, int K, int Hin, int Win,
                     int Cout, int KH, int KW, int OH, int OW, int n_taps, const int* u, const int* v, int pad_h, int pad_w,
                     float* ws, size_t ws_floats, void* stream);
int pg_code_conv_wgrad_plan(int N, int K, int Hin, int Win, int* max_chunks, int* items);
size_t pg_code_conv_wgrad_workspace_floats(int N, int K, int Hin, int Win, int Cout, int KH, int KW);
int pg_code_conv_wgrad(const float* levels, const float* dy, float* dw, float* db, int accumulate, int N, int K, int Hin,
                       int Win, int Cout, int KH, int KW, int OH, int OW, int pad_h, int pad_w, float* ws, size_t ws_floats,
                       void* stream);
int pg_sample_embed_codes(const float* canvas, const float* w, const float* b, const float* pos_term, float* out, int N,
                          int K, int H, int W, int Cout, int KH, int KW, int r, int c, int ld, const int* pos_dev,
                          void* stream);
int pg_vq_lookup(const float* levels, const float* embedding, float* out, int N, int D, int L, int K, void* stream);

/* ---------------------------------------------------------------------------------------
 * Upsampling lookup over an image of code indices, code_up.hip: F.conv_transpose2d(one_hot(codes), w, stride = f) with
 * kernel = stride = f as a table lookup with a phase — how an autoregressive prior over the bottom codes of a two-level
 * VQ-VAE takes the top codes as context (nn.CodeUpsample, ImageGPT.set_condition). levels (N, 1, h, w) dense: a code image
 * as above (a NEGATIVE level adds nothing); w (K, Cout, f, f), the nn.ConvTranspose2d layout; the output image is
 * (N, Cout, h f, w f).
 *   fwd:    out[n, co, i f + a, j f + b] = base[n, co, i f + a, j f + b] + w[code(n, i, j), co, a, b]. base may be NULL (the
 *           lookup alone) and out may BE base (the conditioned stem in one pass: every element is read and written by one
 *           thread, once). The weight is packed once per call into (f f, K, Cout) rows in `ws`
 *           (pg_code_up_fwd_workspace_floats floats). One fp32 addition per element: bit-reproducible.
 *   wgrad:  dw[k, co, a, b] (+)= sum of dy[n, co, i f + a, j f + b] over the top positions with code(n, i, j) = k.
 *           Store-and-sum as pg_code_conv_wgrad, over the inverted index of the N h w TOP positions: one wave sums a chunk
 *           of at most 512 list entries for a group of channels (lanes = channel x phase), a code's chunks are added in
 *           chunk order. No float atomics, no host synchronisation, capturable; bit-reproducible. Codes that never occur
 *           receive exact zeros. accumulate != 0 adds the finished sum to dw (a flat-gradient sink) with one fp32 addition
 *           per element. ws: pg_code_up_wgrad_workspace_floats floats.
 *   plan:   host only. max_chunks = ceil(N h w / 512), items = K + N h w / 512, as pg_code_conv_wgrad_plan.
 * pg_sample_cond_codes: the decode-time half. x[co * ld + n] += w[code(n, r / f, c / f), co, r % f, c % f] on the
 *   (Cout, ld) plane pg_sample_embed_codes writes, for raster position (r, c) of the (h f, w f) image (pos_dev != NULL:
 *   the position is read from the device and clamped to the image).
 * K in 2..4096, f in 1..4, any Cout >= 1 (pg_sample_cond_codes: at most 65535), positions and weights below 2^31 (PG_ESHAPE
 * otherwise); PG_EINVAL for a null operand, a pixel outside the image or a short workspace. No device call before these
 * checks; the queries return 0 for shapes the launch refuses. */
size_t pg_code_up_fwd_workspace_floats(int K, int Cout, int f);
int pg_code_up_fwd(const float* levels, const float* w, const float* base, float* out, int N, int K, int h, int wd, int Cout,
                   int f, float* ws, size_t ws_floats, void* stream);
int pg_code_up_plan(int N, int K, int h, int wd, int* max_chunks, int* items);
size_t pg_code_up_wgrad_workspace_floats(int N, int K, int h, int wd, int Cout, int f);
int pg_code_up_wgrad(const float* levels, const float* dy, float* dw, int accumulate, int N, int K, int h, int wd, int Cout,
                     int f, float* ws, size_t ws_floats, void* stream);
int pg_sample_cond_codes(const float* cond_levels, const float* w, float* x, int N, int K, int h, int wd, int Cout, int f,
                         int r, int c, int ld, const int* pos_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PG_HIP_H_ */
