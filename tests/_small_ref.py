"""Float64 references and shared inputs for the small kernels between the large ones (csrc/elementwise.hip,
csrc/layernorm.hip, the pooling / resampling / phase half of csrc/vae_ops.hip, pg_mse_* of csrc/vq.hip) — plain torch,
no GPU. tests/test_small_ref_cpu.py pins the references and vets the inputs, tests/test_gpu_small_kernels.py compares
the kernels with them through the C-ABI.

Every numeric reference is the formula of the kernel's header comment, evaluated in `dtype` (float64 by default) on the
float32 inputs upcast; `dtype=torch.float32` is the same statement in float32, which the CPU tier uses to show that a
correct float32 evaluation of each input set stays inside the bound the GPU tier applies. The data-movement references
are index formulas written with reshape / slicing. Three kernels do one or two IEEE float32 operations in a stated
order (avgpool2 forward, upsample backward, pg_sum_rows): their reference is that order in float32, bit for bit."""

import math

import torch

SENTINEL = -12345.678             # finite: torch.equal works
PAD = 8                           # sentinel floats in front of and behind every output region (a multiple of 4: the
#                                   region stays 16-byte aligned when the buffer is)
F32_TINY = 2.0 ** -126
ACT_RELU, ACT_ELU, ACT_GELU = 1, 2, 3
GATE_TANH, GATE_IDENTITY = 0, 1
GATES = {"tanh": GATE_TANH, "identity": GATE_IDENTITY}
LN_EPS = 1e-5

# Largest |float32 restatement - float64| on the very inputs the GPU tier uses (measured by and asserted in
# tests/test_small_ref_cpu.py: tests/test_cpu_gelu.py's gelu_parts for GELU, a plain float32 evaluation of the
# functions below for the others). The GPU tier's element-wise absolute bound is ABS_FACTOR times the figure: the
# kernels use the hardware exp2 / reciprocal approximations, one ulp where numpy's are correctly rounded. Each constant
# is the measurement rounded up by 7 to 12 %: the CPU tier asserts that the measurement lies within [0.5, 1] of it, and
# torch's float32 exp / tanh may round a few elements differently on a CPU with another vector width.
ABS_FACTOR = 4.0
CPU_ABS_ERR = {
    "elu_fwd": 5.0e-8, "elu_bwd": 2.6e-7, "elu_bwd_out": 2.5e-7,
    "gelu_fwd": 4.6e-7, "gelu_bwd": 9.4e-7,
    "gated_tanh_fwd": 1.6e-7, "gated_tanh_fwd_res": 3.5e-7, "gated_tanh_bwd": 7.5e-7,
    "gated_identity_fwd": 1.0e-6, "gated_identity_fwd_res": 1.45e-6, "gated_identity_bwd": 1.15e-6,
    "concat_elu_fwd": 5.0e-8, "concat_elu_bwd": 4.5e-7,
}


def gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------
# activations
def relu(x, dtype=torch.float64):
    x = x.to(dtype)
    return torch.where(x > 0, x, torch.zeros_like(x))


def relu_grad(x, dtype=torch.float64):
    return (x > 0).to(dtype)


def elu(x, dtype=torch.float64):
    """x > 0 ? x : exp(x) - 1."""
    x = x.to(dtype)
    return torch.where(x > 0, x, torch.exp(x) - 1.0)


def elu_grad(x, dtype=torch.float64):
    """x > 0 ? 1 : exp(x)."""
    x = x.to(dtype)
    return torch.where(x > 0, torch.ones_like(x), torch.exp(x))


def elu_grad_from_out(y, res=None, dtype=torch.float64):
    """ELU's derivative recovered from its OUTPUT v = y - res: v > 0 ? 1 : v + 1."""
    v = y.to(dtype) if res is None else y.to(dtype) - res.to(dtype)
    return torch.where(v > 0, torch.ones_like(v), v + 1.0)


def relu_grad_from_out(y, res=None, dtype=torch.float64):
    v = y.to(dtype) if res is None else y.to(dtype) - res.to(dtype)
    return (v > 0).to(dtype)


def _phi(x):
    return 0.5 * torch.erfc(-x * math.sqrt(0.5))       # (1 + erf(x / sqrt 2)) / 2 without the cancellation for x < 0


def gelu(x, dtype=torch.float64):
    x = x.to(dtype)
    return x * _phi(x)


def gelu_grad(x, dtype=torch.float64):
    x = x.to(dtype)
    return _phi(x) + x * torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))


ACT_FWD = {"relu": relu, "elu": elu, "gelu": gelu}
ACT_GRAD = {"relu": relu_grad, "elu": elu_grad, "gelu": gelu_grad}
ACT_ID = {"relu": ACT_RELU, "elu": ACT_ELU, "gelu": ACT_GELU}


def sigmoid(b):
    """1 / (1 + exp(-b)) with the exponential of -|b| only: no overflow, and sigmoid(-30) = 9.4e-14 keeps every digit."""
    e = torch.exp(-b.abs())
    return torch.where(b >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def gated_fwd(x, gate, res=None, dtype=torch.float64):
    """x (N, 2 C, L) -> (N, C, L): f(a) sigmoid(b) (+ res), a / b the channel halves, f = tanh or the identity."""
    x = x.to(dtype)
    C = x.shape[1] // 2
    a, b = x[:, :C], x[:, C:]
    y = (torch.tanh(a) if gate == GATE_TANH else a) * sigmoid(b)
    return y if res is None else y + res.to(dtype)


def gated_bwd(x, dy, gate, dtype=torch.float64, mutate=False):
    """dx (N, 2 C, L): da = g f'(a) s, db = g f(a) s (1 - s), 1 - s taken as sigmoid(-b). `mutate` plants the error
    `s` for `1 - s` (the CPU tier's mutation check)."""
    x, g = x.to(dtype), dy.to(dtype)
    C = x.shape[1] // 2
    a, b = x[:, :C], x[:, C:]
    s, one_minus_s = sigmoid(b), sigmoid(-b)
    if mutate:
        one_minus_s = s
    if gate == GATE_TANH:
        f = torch.tanh(a)
        df = 1.0 - f * f
    else:
        f, df = a, torch.ones_like(a)
    return torch.cat((g * df * s, g * f * s * one_minus_s), dim=1)


def concat_elu_fwd(x, dtype=torch.float64):
    """x (N, C, L) -> (N, 2 C, L) = [elu(x) | elu(-x)]."""
    return torch.cat((elu(x, dtype), elu(-x, dtype)), dim=1)


def concat_elu_bwd(x, dy, dtype=torch.float64):
    C = x.shape[1]
    g = dy.to(dtype)
    return g[:, :C] * elu_grad(x, dtype) - g[:, C:] * elu_grad(-x, dtype)


# ---------------------------------------------------------------------------------------------
# losses
def bce(z, x, dtype=torch.float64):
    """z, x (N, per): mean over n of sum_i max(z, 0) - z x + log1p(exp(-|z|))."""
    z, x = z.to(dtype), x.to(dtype)
    return (torch.clamp_min(z, 0.0) - z * x + torch.log1p(torch.exp(-z.abs()))).sum(dim=1).mean()


def bce_grad(z, x, g, dtype=torch.float64):
    """g / N (sigmoid(z) - x)."""
    z, x = z.to(dtype), x.to(dtype)
    return (g / z.shape[0]) * (sigmoid(z) - x)


def mse(a, b, dtype=torch.float64):
    d = a.to(dtype) - b.to(dtype)
    return (d * d).mean()


def mse_grad(a, b, g, dtype=torch.float64):
    """-> (da, db) = (+, -) 2 g / n (a - b)."""
    d = (2.0 * g / a.numel()) * (a.to(dtype) - b.to(dtype))
    return d, -d


# ---------------------------------------------------------------------------------------------
# LayerNorm over C of (N, C, L), biased variance
def layernorm(x, gamma, beta, dy, dx_add=None, eps=LN_EPS, dtype=torch.float64, unbiased=False):
    """-> dict(y, mean (N, L), rstd (N, L), dx, dgamma, dbeta, dx_res = dx + dx_add). `unbiased` plants the error of
    dividing the sum of squares by C - 1 (the CPU tier's mutation check)."""
    x, gamma, beta, dy = (t.to(dtype) for t in (x, gamma, beta, dy))
    C = x.shape[1]
    mean = x.mean(dim=1, keepdim=True)
    var = ((x - mean) ** 2).sum(dim=1, keepdim=True) / (C - 1 if unbiased else C)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean) * rstd
    gc, bc = gamma.reshape(1, C, 1), beta.reshape(1, C, 1)
    g = dy * gc
    dx = rstd * (g - g.mean(dim=1, keepdim=True) - xhat * (g * xhat).mean(dim=1, keepdim=True))
    out = {"y": xhat * gc + bc, "mean": mean.squeeze(1), "rstd": rstd.squeeze(1), "dx": dx,
           "dgamma": (dy * xhat).sum(dim=(0, 2)), "dbeta": dy.sum(dim=(0, 2))}
    out["dx_res"] = dx if dx_add is None else dx + dx_add.to(dtype)
    return out


# ---------------------------------------------------------------------------------------------
# broadcast add
def bcast_colsum(dy, dtype=torch.float64, drop_last=False):
    """dy (N, per) -> (per,): the column sum over the batch. `drop_last` plants the error of a dropped last row."""
    d = dy.to(dtype)
    return (d[:-1] if drop_last else d).sum(dim=0)


def bcast_bwd_bound(dy, start):
    """Per column: (N - 1) 2^-24 sum_n |dy[n, i]| + one ulp of the accumulated start value — the first-order bound of
    a float32 sum of N terms in ANY order, plus the final rounding of start + sum."""
    N = dy.shape[0]
    total = start.double() + dy.double().sum(dim=0)
    ulp = 2.0 ** (torch.floor(torch.log2(total.abs().clamp_min(F32_TINY))) - 23)
    return (N - 1) * 2.0 ** -24 * dy.double().abs().sum(dim=0) + ulp


# ---------------------------------------------------------------------------------------------
# data movement: index formulas
def copy_rows(src, dst, rows, row_len, src_stride, dst_stride, accumulate):
    """Flat float32 buffers; -> the new dst: dst[r ds + i] (+)= src[r ss + i]."""
    out = dst.clone()
    for r in range(rows):
        s = src[r * src_stride:r * src_stride + row_len]
        d = out[r * dst_stride:r * dst_stride + row_len]
        out[r * dst_stride:r * dst_stride + row_len] = d + s if accumulate else s
    return out


def sum_rows(rows):
    """rows: list of (n_batch, per) float32 tensors -> s = 0; s += row_k in ascending order, in float32."""
    s = torch.zeros_like(rows[0])
    for r in rows:
        s = s + r
    return s


def avgpool2_fwd(x):
    """x (planes, 2 OH, 2 OW) float32 -> 0.25f * ((a + b) + (c + d)) in float32, a b the upper pair, c d the lower."""
    a, b, c, d = x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]
    return torch.tensor(0.25, dtype=x.dtype) * ((a + b) + (c + d))


def upsample2_bwd(dy):
    """dy (planes, 2 IH, 2 IW) float32 -> (a + b) + (c + d) in float32."""
    a, b, c, d = dy[:, 0::2, 0::2], dy[:, 0::2, 1::2], dy[:, 1::2, 0::2], dy[:, 1::2, 1::2]
    return (a + b) + (c + d)


def upsample2_fwd(x):
    """x (planes, IH, IW) -> (planes, 2 IH, 2 IW), y[2 r + i, 2 c + j] = x[r, c]."""
    p, h, w = x.shape
    return x.reshape(p, h, 1, w, 1).expand(p, h, 2, w, 2).reshape(p, 2 * h, 2 * w).clone()


def avgpool2_bwd(dy, res=None):
    """0.25f * dy[r, c] at the four pixels of its block (one exact float32 product), + res (one float32 sum)."""
    v = upsample2_fwd(torch.tensor(0.25, dtype=dy.dtype) * dy)
    return v if res is None else v + res


def phase_split(x):
    """x (planes, 2 H, 2 W) -> (4, planes, H, W): xs[2 pr + pc][plane][r][c] = x[plane][2 r + pr][2 c + pc]."""
    return torch.stack([x[:, pr::2, pc::2] for pr in (0, 1) for pc in (0, 1)]).contiguous()


def col_subsample2(x):
    """x (rows, W) -> (rows, W / 2): y[row][q] = x[row][2 q]."""
    return x[:, 0::2].contiguous()


def col_zero_insert2(x):
    """x (rows, W) -> (rows, 2 W): y[row][2 q] = x[row][q], y[row][2 q + 1] = 0."""
    y = torch.zeros(x.shape[0], 2 * x.shape[1], dtype=x.dtype)
    y[:, 0::2] = x
    return y


# ---------------------------------------------------------------------------------------------
# shared inputs
# -90: exp underflows. Values of order 1 come first: the smallest sizes hold only these, and the max-normalised bound is
# then relative to an output of order 1 (next to 1e-3 alone, the float32 rounding of exp(x) - 1 is 3e-5 of the maximum)
ACT_SPECIALS = (-8.0, 20.0, 0.0, -1e-3, F32_TINY, -F32_TINY, 1e-3, 8.0, -20.0, -90.0)
EW_CAP = 4096 * 256               # threads of a capped elementwise / pooling grid: more items than this loop
ACT_N = (1, 3, 4, 5, 255 * 4 + 1, 1024 * 4)
ACT_N_BIG_ALIGNED = 4 * EW_CAP + 7     # 1048577 float4 items (grid-stride) and a tail of 3
ACT_N_BIG_UNALIGNED = EW_CAP + 3       # scalar path, grid-stride
FROM_OUT_N = (4, 1028, 4 * EW_CAP + 4)
GATED_VEC = ((1, 1, 4), (2, 3, 8), (3, 5, 64))
GATED_SCALAR = ((2, 3, 7),)            # and (2, 3, 8) on an unaligned base
GATED_BIG = (2, 3, 699052)             # N C L / 4 = 1048578 float4 items
CONCAT_ELU = ((1, 1), (3, 35), (3, 349527))          # (N, C L); the last: 1048581 items
BCAST_N = (1, 2, 31, 32, 33, 224, 225, 257, 513)
BCAST_PER = (1, 31, 32, 33, 100)
# the four corners, and a walk that meets every N and every per (N > 224 runs the 8-loads-in-flight loop)
BCAST_CASES = ((1, 1), (1, 100), (513, 1), (513, 100), (2, 31), (31, 32), (32, 33), (33, 100), (224, 33), (225, 32),
               (257, 31), (225, 100), (257, 1))
BCE_CASES = ((1, 1), (3, 255), (4, 784), (5, 26215))  # the last: 131075 > 512 * 256 elements
MSE_N = (1, 255, 1000, 2048 * 256 + 3)                # the last: past the forward's 512 blocks and the backward's 2048
COPY_BIG = (3, 699051)                                # rows, row_len: 2097153 > 8192 * 256 scalar items
SUM_ROWS_N = (1, 2, 32)
SUM_ROWS_SHAPES = ((1, 1), (3, 50), (2, 600))
POOL_SHAPES = ((1, 1, 1), (3, 2, 5), (6, 7, 3), (3, 592, 591))    # the last: 1049616 > 4096 * 256 pooled pixels
PHASE_SHAPES = ((1, 1, 1), (3, 2, 5), (4, 5, 3), (3, 296, 297))   # the last: 1054944 elements of x
COL_ROWS, COL_W = (1, 7), (2, 6, 34)
COL_BIG = (61681, 34)                                 # 61681 * 17 = 1048577 sub-sampled elements
LN_C = (1, 2, 16, 17, 32, 33, 64, 65)
LN_NL = ((1, 1), (3, 49), (1, 513))
LN_G_CASES = ((5, 3277), (3, 10923), (13, 3781))      # N L = 16385, 32769, 49153: G = 33, 65, 97 partial rows (C = 17)
LN_RES_C = (16, 17, 33)


def act_inputs(n, salt=0):
    """-> (x, dy): x random (scale 2.5) with x[0] = -0.5 (so that the smallest sizes have an output of order 1 on the
    exponential branch) and the special values planted behind it, as many as fit — at a stride of 3 from n = 32 on, so
    that a float4 holds specials and random values side by side."""
    g = gen(n, salt, 11)
    x = 2.5 * torch.randn(n, generator=g)
    x[0] = -0.5
    step = 3 if n >= 32 else 1
    for k, v in enumerate(ACT_SPECIALS):
        if 1 + k * step < n:
            x[1 + k * step] = v
    return x, torch.randn(n, generator=g)


def from_out_inputs(n, act, with_res, salt=0):
    """-> (y, res or None, dy): y = act(pre) + res in float32, with pre planted at 0 (y exactly res) and at values
    whose output is exactly 0 + res."""
    g = gen(n, act, with_res, salt, 13)
    pre = 2.0 * torch.randn(n, generator=g)
    pre[0], pre[n // 2], pre[n - 1] = 0.0, 0.0, -0.0
    out = (elu(pre, torch.float32) if act == ACT_ELU else relu(pre, torch.float32))
    res = torch.randn(n, generator=g) if with_res else None
    y = out + res if with_res else out
    return y, res, torch.randn(n, generator=g)


def gated_inputs(N, C, L, salt=0):
    """-> (x (N, 2 C, L), dy (N, C, L), res (N, C, L)): a ~ 2 N(0, 1), b ~ 4 N(0, 1), with |b| = 30 and |a| = 10
    planted in every combination of signs at the first four elements of sample 0 — or the first half of them, where the
    sample has fewer than eight (every gradient at a planted element is below 1e-8: some ordinary ones stay beside them)."""
    g = gen(N, C, L, salt, 17)
    x = torch.randn(N, 2 * C, L, generator=g)
    x[:, :C] *= 2.0
    x[:, C:] *= 4.0
    flat_a, flat_b = x[0, :C].reshape(-1), x[0, C:].reshape(-1)      # views: C L elements of sample 0
    for k, (a, b) in enumerate(((10.0, 30.0), (-10.0, -30.0), (10.0, -30.0), (-10.0, 30.0))):
        if 2 * k < flat_a.numel():
            flat_a[k], flat_b[k] = a, b
    return x, torch.randn(N, C, L, generator=g), torch.randn(N, C, L, generator=g)


def bcast_inputs(N, per):
    """-> (x, p, dy, the start value of dp). For N <= 2 dy and the start are multiples of 1 / 64: the sum is then exact in
    float32 — the bound of the backward is the two roundings themselves there, which no float32 sum of arbitrary values
    undercuts by a factor 2."""
    g = gen(N, per, 19)
    x, p, dy = torch.randn(N, per, generator=g), torch.randn(per, generator=g), torch.randn(N, per, generator=g)
    start = 3.0 * torch.randn(per, generator=g) + 0.5
    if N <= 2:
        dy, start = torch.round(dy * 64.0) / 64.0, torch.round(start * 64.0) / 64.0
    return x, p, dy, start


def bce_inputs(N, per, fractional=False):
    """-> (z, x): logits ~ 3 N(0, 1) with +-40 planted, targets in {0, 1} (or uniform in [0, 1])."""
    g = gen(N, per, fractional, 23)
    z = 3.0 * torch.randn(N, per, generator=g)
    zf = z.reshape(-1)
    for k, v in enumerate((40.0, -40.0, 0.0)):
        if k + 1 < zf.numel():
            zf[k + 1] = v
    u = torch.rand(N, per, generator=g)
    return z, (u if fractional else (u < 0.4).float())


def mse_inputs(n):
    g = gen(n, 29)
    return torch.randn(n, generator=g), torch.randn(n, generator=g) + 0.25


def ln_inputs(N, C, L, salt=0):
    """-> (x, gamma, beta, dy, dx_add): x = 3 N(0, 1) + 0.5, as tests/test_gpu_ops.py feeds the operator. C = 2 is the
    exception, x = 0.01 N(0, 1): with two channels xhat = +-h and dx = rstd (g_1 - g_2) / 2 (1 - h^2) with
    1 - h^2 = eps / (var + eps) — at a variance of 9 that is 1e-6, and dx is what float32 rounding leaves of a
    cancellation (a float32 evaluation misses the bound 100-fold); at a variance of 1e-4 it is 0.1."""
    g = gen(N, C, L, salt, 31)
    x = 3.0 * torch.randn(N, C, L, generator=g) + 0.5
    if C == 2:
        x = 0.01 * torch.randn(N, C, L, generator=g)
    return (x, torch.randn(C, generator=g) + 1.0, torch.randn(C, generator=g), torch.randn(N, C, L, generator=g),
            torch.randn(N, C, L, generator=g))


LN_ZERO_VAR_C = (16, 64, 128)        # powers of two: the float32 mean of C copies of 0.75 is exactly 0.75


def ln_zero_variance_inputs(C):
    """(N, L) = (2, 7) with pixel (1, 3) holding 0.75 in every channel: zero variance there, rstd = 1 / sqrt(eps)."""
    x, gamma, beta, dy, dx_add = ln_inputs(2, C, 7, salt=1)
    x[1, :, 3] = 0.75
    return x, gamma, beta, dy, dx_add


def rand(*shape, salt=0):
    return torch.randn(*shape, generator=gen(*shape, salt, 37))
