// conv_wgrad_route.h — the route of pg_conv2d_wgrad: ONE host function (conv_wgrad.hip: wgrad_route) decides which of the six kernel
// families takes a weight-gradient problem and how it is laid out. The launch (pg_conv2d_wgrad) and the host-only export
// pg_conv2d_wgrad_route both read its answer, like b3_route (conv_b3.hip) for the forward convolution.
//
// A family's plan function (pg_wgrad_*_plan) is pure host arithmetic on a WgProblem: it either declines (returns 0) or fills the
// WgRoute — the figures the export reports AND the family's kernel arguments with every pointer still null. The family's run function
// (pg_wgrad_*_run) takes that route, sets the pointers and launches the instantiation the route names; it decides nothing.
#pragma once
#include "common.h"

struct WgProblem {
  int N, Cin, IH, IW, Cout, OH, OW, KH, KW, T;
  const int* tap_dr;
  const int* tap_dc;
  int in_act;
  bool has_bias;         // db given: one more slot row per output channel
  bool x_al16, dy_al16;  // x / dy 16-byte aligned (every fast family declines otherwise)
  long stride;           // floats per partial row = Cout * Cin * T + Cout
  long max_rows;         // partial rows the workspace holds (wgrad_max_rows)
};

enum WgFamily { WGF_XCOPY = 0, WGF_RING = 1, WGF_SHIFTED = 2, WGF_PW = 3, WGF_SMALL = 4, WGF_GENERIC = 5 };

// ---- kernel arguments of the six families (documented next to their kernels) -----------------------------------------------------
constexpr int WB_MAXT = 9;
constexpr int SW_COLS = 64;

struct WbArgs {  // conv_wgrad_b3_kernel (x-copy bf16x3)
  const float* x; const float* dy; float* part;
  long part_stride;
  int N, Cin, Cout, H, W, T;
  int TR, xh, tiles_per_img, total_tiles, min_dr;
  int PBR, dpb, xpb, ksteps;   // pixel blocks per row / per dy tile / per x tile; K steps per tile
  int dslots, xslots;
  int ndc, dcs[3];             // distinct column shifts (copies)
  int x_off16;                 // first 16-byte entry of the x area
  int in_act, has_bias;
  int dbg;                     // ablation switches (PG_WB_DBG: 1 no loads, 2 no commit, 4 no MFMA), 0 in production
  int tap_base[WB_MAXT];       // entry offset of tap t inside the x area: copy plane + row-shift blocks
};

struct WrArgs {  // conv_wgrad_b3r_kernel (row ring)
  const float* x; const float* dy; float* part;
  long part_stride;
  int N, Cin, Cout, H, W, T;
  int nseg, seg_rows, units;   // row segments per image, rows per segment, N * nseg work units (strided over blockIdx.x)
  int P, RB;                   // x-only steps in front of a segment (= hr), ring rows (= hr + 1)
  int max_dr;
  int ndc, dcs[3];             // distinct column shifts (copies)
  int x_off16;                 // first 16-byte entry of the x area
  int in_act, has_bias;
  int dbg;                     // ablation switches (PG_WB_DBG: 1 no loads, 2 no commit, 4 no MFMA, 8 no fragment reads either), 0 in production
  int copy_of[6], q_of[6];     // per tap: its x copy; rows back from the newest ring row (max_dr - dr)
};

struct WsArgs {  // conv_wgrad_b3s_kernel (shifted dy)
  const float* x; const float* dy; float* part;
  long part_stride;
  int N, Cin, Cout, H, W, T;
  int TR, xh, tiles_per_img, total_tiles, min_dr, min_dc;
  int PBR, dpb, xpb, ksteps;
  int dslots, xslots;
  int x_off16;                 // first 16-byte entry of the x area (behind NC dy copies x 3 pieces)
  int v0;                      // dy copy with dc == 0 (bias sums)
  int wpart;                   // W % 8 != 0: the last pixel block of a row holds 4 pixels
  int in_act, has_bias;
  int tap_of[9];               // caller's tap index of grid position (ri, ci): ri * NC + ci
};

struct SwArgs {  // conv_wgrad_small_kernel (input layers)
  const float* x; const float* dy; float* part;
  long part_stride;
  int N, Cin, Cout, H, W, T;
  int TR, tiles_per_img, total_tiles;
  int min_dr, min_dc, tile_w, xrows;   // x tile: xrows x tile_w per channel, origin (row0 + min_dr, min_dc)
  int dstride;                         // dy tile row stride (floats), TR * W + pad
  int ncols, bias_col;                 // used columns (Cin * T [+ 1]); index of the ones column or -1
  int in_act;
  int col_off[SW_COLS];                // LDS float offset of column j inside the x tile (ci plane + tap shift); -1: unused
};

struct WgArgs {  // conv_wgrad_kernel (generic fp32)
  const float* x; const float* dy; float* dw; float* db;
  float* part;        // [gridDim.x][part_stride] per-block partial sums (no atomics: see below)
  long part_stride;   // = Cout*Cin*T + Cout
  int N, Cin, IH, IW, Cout, OH, OW, KH, KW, T;
  int TR, tiles_per_img, total_tiles, SW, xh, min_dr, min_dc;
  int S_dy, S_x, npos, in_act;
  int swp_shift, rpi;       // lanes per staged row = 1<<swp_shift, rows per wave iteration
  int dump;                 // LDS float index of the dump word (past every tile / scratch area)
  int vec_dy, vec_x, qshift_dy, qshift_x;  // float4 staging when rows are 16-byte aligned
  float inv_TR, inv_xh;
  int prefetch;             // float4 slot staging with register prefetch (both tensors 16-byte aligned rows)
  int Qd, Qx, dslots, xslots;  // quads per row and slots per tile (dy / x)
  int tapoff[PG_MAX_TAPS];
  int tap_u[PG_MAX_TAPS];
  int tap_v[PG_MAX_TAPS];
};

struct PwWgArgs {  // conv_wgrad_pw_kernel (fp32 1x1)
  const float* x; const float* dy; float* dw; float* db;
  float* part;        // [gridDim.x][Cout*Cin + Cout]
  long part_stride;
  int N, Cin, Cout, L, G16, in_act;
  long total_groups;
};

// ---- the route -----------------------------------------------------------------------------------------------------------------------
struct WgRoute {
  int family;     // WgFamily
  int t[4];       // the instantiation: x-copy T, MR, waves, CIT | ring T, WM, WN | shifted-dy NR, NC | 1x1 NCOT, NCIT, ACT |
                  // input layer - | generic NT, NC, prefetch
  int gx, gy, gz, block;
  size_t shmem;   // dynamic LDS bytes
  int G;          // partial rows written = rows the reduction reads (= gx)
  int TR, tiles_per_img;
  long total;     // tiles (x-copy, shifted-dy, input layer, generic), (image, segment) units (ring), 16-pixel groups (1x1)
  int nseg, seg_rows, PBR, vec_dy, vec_x;
  int hr, copies, passes;  // row halo of the tap list; x copies (x-copy, ring) or dy copies (shifted-dy); tap passes (generic)
  WbArgs wb; WrArgs wr; WsArgs ws; SwArgs sw; WgArgs wg; PwWgArgs pw;  // the chosen family's kernel arguments, pointers null
  char msg[192];  // why no family takes the problem (the launch's error text)
};

// conv_wgrad_b3.hip: x-copy and row-ring kernels (one plan: the ring is tried first inside it), shifted-dy kernel
int pg_wgrad_b3_plan(const WgProblem& p, WgRoute& r);
int pg_wgrad_b3_run(const WgRoute& r, const float* x, const float* dy, float* part, hipStream_t st);
int pg_wgrad_b3s_plan(const WgProblem& p, WgRoute& r);
int pg_wgrad_b3s_run(const WgRoute& r, const float* x, const float* dy, float* part, hipStream_t st);
// conv_wgrad_small.hip: input layers (<= 4 input channels, many taps)
int pg_wgrad_small_plan(const WgProblem& p, WgRoute& r);
int pg_wgrad_small_run(const WgRoute& r, const float* x, const float* dy, float* part, hipStream_t st);
// plan: 1 = the family takes the problem (route filled), 0 = it declines. run: 0, or -1 when the launch failed.
