// gpt_ends.h — the partial-row layouts that gpt_ends.hip (the ImageGPT stem and output head) writes and
// pg_gpt_model_reduce (gpt_block.hip) adds up.
#pragma once

namespace pg_ends {

constexpr int C = 16;            // embedding channels
constexpr int MAX_COUT = 4;      // output-head channels the kernels are instantiated for
constexpr int TAPS = 9, ACTIVE = 4;  // 3x3 taps; the type A mask keeps taps 0..3 (three above, one left)

// output head, one row per workgroup: d ln.weight | d ln.bias | d conv.weight (Cout x 16) | d conv.bias (Cout)
constexpr int O_G = 0, O_BE = O_G + C, O_W = O_BE + C;
constexpr int out_row_floats(int cout) { return O_W + cout * C + cout; }

// stem, region A, one row per workgroup: d weight (16 x 9) | d bias (16)
constexpr int S_W = 0, S_B = S_W + C * TAPS, S_PART = S_B + C;  // 160
// stem, region B, one row per image slice: G[tap][p] = sum_n sum_c w[c][tap] dx0[n][c][p], ACTIVE x L floats; the
// reduce gathers d pos[q] = sum_tap G[tap][q - off(tap)]
constexpr int stem_workspace_floats(int rows, int slices, int L) { return rows * S_PART + slices * ACTIVE * L; }

}  // namespace pg_ends
