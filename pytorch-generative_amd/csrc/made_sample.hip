// made_sample.hip — a whole sample of a one-hidden-layer MADE in ONE launch, on cached hidden sums.
//
// The reference's sampler (made.py:125-141) runs one full masked forward per dimension and uses one logit of it. With one
// hidden layer the hidden pre-activation a = b1 + W1m x changes by the rank-1 update a += x_i W1m[:, i] when dimension i is
// fixed, and the one logit needed is the dot product b2[i] + relu(a) . W2m[i, :] (what NADE does): 4 H flops per dimension
// instead of 4 D H. Nothing crosses samples, and the weight addresses of every step depend on `order` alone, so all D steps
// run inside one kernel with no grid-wide synchronisation:
//   * one workgroup owns a tile of MS_TILE samples; `a` of the tile lives in registers, U consecutive hidden units per thread,
//     for all D steps;
//   * row i of W2m and of the TRANSPOSED W1m come from a pack made once per call (pg_made_sample_pack), side by side and
//     zero-padded to Hp = threads * U floats, so a step reads one contiguous 2 Hp float chunk with no bounds check, once per
//     workgroup for all samples of the tile;
//   * the rows, the bias, the canvas entries and the uniforms of step s + 1 are issued before the reduce, the draw and the
//     update of step s, into the other of two operand sets (no copy, so each is waited for where step s + 1 uses it); `order`
//     stays in registers, 64 steps to a wave: a step is one reduction and one barrier deep and addresses no memory it waits for;
//   * measured on the recipe's 784 -> 8000 -> 784 (profiles/made_sampling.json): 1.9 us per dimension, which is one workgroup
//     reading its 64 KB of weight rows at the 34 GB/s one CU gets from the Infinity Cache;
//   * the reduction over H has a fixed order — U units per thread in turn, the lanes of a wave, the waves in turn — that
//     depends on H alone: a sample's rows of canvas and logits_out are bit-identical from run to run, for any N and any slot
//     of the tile. No float atomics.
#include "common.h"

namespace {

constexpr int MS_TILE = 4;        // samples per workgroup
constexpr int MS_MAX_H = 8192;

// The one function that decides the domain and the geometry: pg_made_sample_plan reports it, the pack and the launch go by it.
struct MsPlan {
  int waves, threads, units, hp, grid;
  long pack_floats;
  char msg[160];
};

#define MS_REQUIRE(cond, code, ...)                  \
  do {                                               \
    if (!(cond)) {                                   \
      snprintf(pl.msg, sizeof(pl.msg), __VA_ARGS__); \
      return (code);                                 \
    }                                                \
  } while (0)

int ms_plan(int D, int H, int N, MsPlan& pl) {
  pl.msg[0] = 0;
  MS_REQUIRE(D > 0 && H > 0 && N > 0, PG_EINVAL, "pg_made_sample: non-positive dimension");
  MS_REQUIRE(H <= MS_MAX_H, PG_ESHAPE, "pg_made_sample: %d hidden units unsupported (at most %d)", H, MS_MAX_H);
  // (waves, hidden units per thread): the smallest workgroup that holds H, then wider threads
  if (H <= 64) { pl.waves = 1; pl.units = 1; }
  else if (H <= 256) { pl.waves = 4; pl.units = 1; }
  else if (H <= 1024) { pl.waves = 4; pl.units = 4; }
  else if (H <= 4096) { pl.waves = 16; pl.units = 4; }
  else { pl.waves = 16; pl.units = 8; }
  pl.threads = 64 * pl.waves;
  pl.hp = pl.threads * pl.units;
  pl.pack_floats = 2L * D * pl.hp;
  MS_REQUIRE(pl.pack_floats < (1L << 31), PG_ESHAPE, "pg_made_sample: a pack of %ld floats for D = %d, H = %d is too large",
             pl.pack_floats, D, H);
  pl.grid = pg_cdiv(N, MS_TILE);
  return 0;
}

// The operands as kernel parameters. b2, canvas and uniforms are NOT __restrict__: a load the compiler can prove untouched by
// the canvas stores goes through the scalar cache, whose results return out of order and are waited for with the LDS traffic
// of the reduction; as vector loads the operands of step s + 1 stay in flight, in order, behind those of step s.
#define MS_PARAMS                                                                                                 \
  const float *__restrict__ pack, const float *__restrict__ b1, const float *b2, const int *order, float *canvas, \
      const float *uniforms, float *logits, int N, int D, int H, int hp

template <int CTRL>
__device__ __forceinline__ float ms_dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}

// Sum over the 64 lanes without LDS, the same bits in every lane: lane ^ 1 and lane ^ 2 inside a quad, the mirror of 8 and the
// mirror of 16 lanes on the DPP path (every lane of a 16-lane row then holds the row's sum), then the four row sums in order.
__device__ __forceinline__ float ms_wave_sum(float v) {
  v += ms_dpp<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v += ms_dpp<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v += ms_dpp<0x141>(v);  // row_half_mirror
  v += ms_dpp<0x140>(v);  // row_mirror
  const int b = __float_as_int(v);
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(b, 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(b, 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(b, 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(b, 48));
  return (r0 + r1) + (r2 + r3);
}

template <int U>
__device__ __forceinline__ void ms_load_units(const float* __restrict__ p, float (&v)[U]) {
  if constexpr (U == 1) {
    v[0] = p[0];
  } else {
#pragma unroll
    for (int q = 0; q < U / 4; ++q) {
      const float4 f = reinterpret_cast<const float4*>(p)[q];
      v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w;
    }
  }
}

// What a step reads: its two weight rows (this thread's units), the output bias and, per sample of the tile, the canvas entry
// and the uniform.
template <int U>
struct MsStep {
  float w2[U], w1[U], bias, given[MS_TILE], u[MS_TILE];
};

template <int U>
__device__ __forceinline__ void ms_load_step(const float* __restrict__ pack, const float* b2, const float* canvas,
                                             const float* uniforms, int hp, int i, int unit0,
                                             const size_t (&row)[MS_TILE], MsStep<U>& st) {
  const float* __restrict__ p = pack + (size_t)i * 2 * hp + unit0;
  ms_load_units<U>(p, st.w2);
  ms_load_units<U>(p + hp, st.w1);
  st.bias = b2[i];
#pragma unroll
  for (int t = 0; t < MS_TILE; ++t) {
    st.given[t] = canvas[row[t] + i];
    st.u[t] = uniforms[row[t] + i];
  }
}

// `order` in registers, 64 steps to a wave: lane j of `a` holds the dimension of step 64 c + j of the current chunk c, `b` that
// of chunk c + 1 (loaded 64 steps before its first use); a step reads its dimension with v_readlane, no memory in the loop.
struct MsOrder {
  int a, b;
};
__device__ __forceinline__ int ms_order_chunk(const int* order, int D, int s0, int lane) {
  const int i = order[s0 + lane < D ? s0 + lane : D - 1];
  return i < 0 ? 0 : (i >= D ? D - 1 : i);  // an entry outside [0, D) must not become an address
}
// the dimension of step q, one of the steps s + 2, s + 3 of a step s of the current chunk (past the last step: any valid one)
__device__ __forceinline__ int ms_dim(const MsOrder& o, int s, int q) {
  return __builtin_amdgcn_readlane((q >> 6) == (s >> 6) ? o.a : o.b, q & 63);
}

template <int U, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) made_sample_kernel(MS_PARAMS) {
  // partial sums of a step, [step parity][sample][wave]: two copies, so that a step needs one barrier (a wave writes parity q
  // again only after the barrier of the step between, which every wave reaches after its reads of q)
  __shared__ __attribute__((aligned(16))) float red[2][MS_TILE][WAVES < 4 ? 4 : WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int unit0 = tid * U;
  const int n0 = blockIdx.x * MS_TILE;
  size_t row[MS_TILE];
#pragma unroll
  for (int t = 0; t < MS_TILE; ++t) {
    const int n = n0 + t < N ? n0 + t : N - 1;  // a slot past N recomputes the last sample and writes nothing
    row[t] = (size_t)n * D;
  }
  if (WAVES < 4 && tid < 2 * MS_TILE * 4) (&red[0][0][0])[tid] = 0.f;  // the float4 reads below see zeros past the last wave
  float a[MS_TILE][U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const float b = unit0 + u < H ? b1[unit0 + u] : 0.f;  // padded units: a = 0 against zero weights
#pragma unroll
    for (int t = 0; t < MS_TILE; ++t) a[t][u] = b;
  }
  MsOrder ord = {ms_order_chunk(order, D, 0, lane), 0};
  int i0 = __builtin_amdgcn_readlane(ord.a, 0), i1 = __builtin_amdgcn_readlane(ord.a, 1);
  MsStep<U> even, odd;  // the operands of even and odd steps: no copy between steps, so a step waits for its loads where it uses them
  ms_load_step<U>(pack, b2, canvas, uniforms, hp, i0, unit0, row, even);
  if (WAVES < 4) __syncthreads();

  // step s on dimension i_cur with the operands `cur`; issues the loads of step s + 1 (dimension i_nxt) into `nxt` first
  auto step = [&](int s, int i_cur, int i_nxt, const MsStep<U>& cur, MsStep<U>& nxt) {
    ms_load_step<U>(pack, b2, canvas, uniforms, hp, i_nxt, unit0, row, nxt);  // at the last step: a harmless re-read
    float part[MS_TILE];
#pragma unroll
    for (int t = 0; t < MS_TILE; ++t) {
      float acc = 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u) acc = fmaf(fmaxf(a[t][u], 0.f), cur.w2[u], acc);
      part[t] = ms_wave_sum(acc);
    }
    float(&rq)[MS_TILE][WAVES < 4 ? 4 : WAVES] = red[s & 1];
    if (lane == 0) {
#pragma unroll
      for (int t = 0; t < MS_TILE; ++t) rq[t][wave] = part[t];
    }
    __syncthreads();
    float x[MS_TILE], l[MS_TILE];
#pragma unroll
    for (int t = 0; t < MS_TILE; ++t) {
      float acc = 0.f;
#pragma unroll
      for (int w = 0; w < (WAVES < 4 ? 4 : WAVES); w += 4) {
        const float4 f = *reinterpret_cast<const float4*>(&rq[t][w]);
        acc = (((acc + f.x) + f.y) + f.z) + f.w;
      }
      l[t] = cur.bias + acc;
      const float p = 1.f / (1.f + __expf(-l[t]));
      x[t] = cur.given[t] >= 0.f ? cur.given[t] : (cur.u[t] < p ? 1.f : 0.f);
#pragma unroll
      for (int u = 0; u < U; ++u) a[t][u] = fmaf(x[t], cur.w1[u], a[t][u]);
    }
    if (tid == 0) {
#pragma unroll
      for (int t = 0; t < MS_TILE; ++t) {
        if (n0 + t < N) {
          canvas[row[t] + i_cur] = x[t];
          if (logits) logits[row[t] + i_cur] = l[t];
        }
      }
    }
  };

  for (int s = 0; s < D; s += 2) {
    if ((s & 63) == 0) {
      if (s) ord.a = ord.b;
      ord.b = ms_order_chunk(order, D, s + 64, lane);
    }
    const int i2 = ms_dim(ord, s, s + 2);
    step(s, i0, i1, even, odd);
    if (s + 1 >= D) break;
    const int i3 = ms_dim(ord, s, s + 3);
    step(s + 1, i1, i2, odd, even);
    i0 = i2;
    i1 = i3;
  }
}

// pack[i][0 .. hp) = W2m[i, :], pack[i][hp .. 2 hp) = W1m[:, i], zeros from H on. 32 x 32 tiles over (i, h); the transpose of
// W1m goes through LDS so that reads (along D) and writes (along h) are both contiguous.
__global__ void __launch_bounds__(256) made_sample_pack_kernel(const float* __restrict__ w1, const float* __restrict__ w2,
                                                               float* __restrict__ pack, int D, int H, int hp) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int h0 = blockIdx.x * 32, i0 = blockIdx.y * 32;
#pragma unroll
  for (int j = 0; j < 32; j += 8) {
    const int h = h0 + ty + j, i = i0 + tx;
    tile[ty + j][tx] = (h < H && i < D) ? w1[(size_t)h * D + i] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 32; j += 8) {
    const int i = i0 + ty + j, h = h0 + tx;  // h < hp: hp is a multiple of 64
    if (i < D) {
      float* dst = pack + (size_t)i * 2 * hp + h;
      dst[0] = h < H ? w2[(size_t)i * H + h] : 0.f;
      dst[hp] = tile[tx][ty + j];
    }
  }
}

template <int U, int WAVES>
void ms_launch(const MsPlan& pl, hipStream_t stream, MS_PARAMS) {
  hipLaunchKernelGGL((made_sample_kernel<U, WAVES>), dim3((unsigned)pl.grid), dim3(64 * WAVES), 0, stream, pack, b1, b2, order,
                     canvas, uniforms, logits, N, D, H, hp);
}

}  // namespace

PG_EXPORT int pg_made_sample_plan(int D, int H, int N, int* out, int out_len) {
  PG_REQUIRE(out && out_len >= PG_MADE_SAMPLE_PLAN_INTS, PG_EINVAL, "pg_made_sample_plan: null pointer or short output array");
  MsPlan pl;
  const int rc = ms_plan(D, H, N, pl);
  if (rc) {
    pg_set_error("%s", pl.msg);
    return rc;
  }
  out[0] = MS_TILE;
  out[1] = pl.threads;
  out[2] = pl.units;
  out[3] = (int)sizeof(float) * 2 * MS_TILE * (pl.waves < 4 ? 4 : pl.waves);
  out[4] = (int)pl.pack_floats;
  out[5] = pl.hp;
  out[6] = pl.grid;
  out[7] = MS_MAX_H;
  return 0;
}

PG_EXPORT int pg_made_sample_pack(const float* w1, const float* w2, float* pack, int D, int H, void* stream) {
  PG_REQUIRE(w1 && w2 && pack, PG_EINVAL, "pg_made_sample_pack: null pointer");
  MsPlan pl;
  const int rc = ms_plan(D, H, 1, pl);
  if (rc) {
    pg_set_error("%s", pl.msg);
    return rc;
  }
  PG_REQUIRE(pg_cdiv(D, 32) <= 65535, PG_ESHAPE, "pg_made_sample_pack: D = %d too large", D);
  hipLaunchKernelGGL(made_sample_pack_kernel, dim3((unsigned)(pl.hp / 32), (unsigned)pg_cdiv(D, 32)), dim3(32, 8), 0,
                     (hipStream_t)stream, w1, w2, pack, D, H, pl.hp);
  PG_LAUNCH_CHECK("pg_made_sample_pack");
  return 0;
}

PG_EXPORT int pg_made_sample(const float* pack, const float* b1, const float* b2, const int* order, float* canvas,
                             const float* uniforms, float* logits_out, int N, int D, int H, void* stream) {
  PG_REQUIRE(pack && b1 && b2 && order && canvas && uniforms, PG_EINVAL, "pg_made_sample: null pointer");
  PG_REQUIRE((uintptr_t)pack % 16 == 0, PG_EINVAL, "pg_made_sample: the pack must be 16-byte aligned");
  MsPlan pl;
  const int rc = ms_plan(D, H, N, pl);
  if (rc) {
    pg_set_error("%s", pl.msg);
    return rc;
  }
  const hipStream_t st = (hipStream_t)stream;
#define MS_ARGS pl, st, pack, b1, b2, order, canvas, uniforms, logits_out, N, D, H, pl.hp
  if (pl.waves == 1) ms_launch<1, 1>(MS_ARGS);
  else if (pl.waves == 4 && pl.units == 1) ms_launch<1, 4>(MS_ARGS);
  else if (pl.waves == 4) ms_launch<4, 4>(MS_ARGS);
  else if (pl.units == 4) ms_launch<4, 16>(MS_ARGS);
  else ms_launch<8, 16>(MS_ARGS);
#undef MS_ARGS
  PG_LAUNCH_CHECK("pg_made_sample");
  return 0;
}
