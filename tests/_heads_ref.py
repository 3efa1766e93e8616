"""Float64 references and shared inputs for the discretized mixture-of-logistics kernels (csrc/dmol.hip) and the
Gaussian-head / small reduction kernels of csrc/vae_ops.hip — plain torch, no GPU. tests/test_heads_ref_cpu.py pins the
references and vets the inputs, tests/test_gpu_dmol_kernels.py and tests/test_gpu_gauss_heads.py compare the kernels
with them through the C-ABI.

DMOL: the reference is oracle/dmol.py (pinned by quadrature in tests/test_dmol_cpu.py) in float64 on the float32
inputs upcast. Pixels are handled as ROWS: `rows` (P, 10 K) holds the 10 K parameters of P independent pixels, `x`
(P, 3) their sub-pixel values; a row is at the same time the kernel's (N = 1, 10 K, L = 1) tensor, and
`to_kernel_layout` turns P rows into (N, 10 K, L). `form` selects how the interior bin mass is written — "stable" is
oracle/dmol.py as it stands (and the kernel), "plain" the earlier sigmoid(pin) - sigmoid(nin) — and `dtype` lets the
CPU tier evaluate the very same statement in float32.

Conventions stated here and not tested: a log-scale of exactly -7.0 sits on the kink of the clamp, where the kernel's
mask (`>`) gives gradient 0 and torch.clamp's backward gives 1 — no input uses it; and the likelihood jumps where the
bin mass crosses MASS_SWITCH, so no input chosen here has a mass within 10 % of it (BAND; the one grid point the tail
sweep is REQUIRED to contain that does, is named in BAND_GRID_POINT and asserted separately)."""

import math

import torch
import torch.nn.functional as F

from oracle import dmol as odmol

BIN = odmol.BIN
LL_TOL = 1e-4                     # the TOL of tests/test_gpu_f4.py, per pixel here
# absolute term of the per-pixel bound: log sigmoid(z) of an edge bin is z - softplus(z) in the kernel and the oracle
# alike, exact to one float32 ulp of |z|; the inputs keep |z| < 128 (ulp 2^-17) and a pixel has three sub-pixels.
# It only matters where |log-likelihood| < 0.23 (saturated edge bins, whose true value is ~ -1e-26).
LL_ABS = 3 * 2.0 ** -17
BAND = (0.9e-5, 1.1e-5)
F32_TINY = 2.0 ** -126
SENTINEL = -12345.678             # finite: torch.equal works
S_SWEEP = (0.5, -1.0, -3.0, math.log(0.01), -6.0, -6.9, -7.1, -9.0)
T_SWEEP = (0.0, 0.3, 2.0, 5.0, 8.0, 9.0, 10.0, 11.0, 12.0, 13.0, 16.0, 25.0, 60.0)
T_MIXED = ((8.0, 0.3, 12.0), (10.0, 2.0, 25.0), (11.0, 60.0, 5.0))   # a different t per sub-pixel
BAND_GRID_POINT = (-6.0, 13.0)    # mass 1.053e-5: 5 % above the switch, five orders above any float32 error of it
MIXTURE_KS = (1, 2, 3, 10, 16)


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------
# DMOL reference
def component_log_probs_plain(x, means, log_scales, coeffs):
    """oracle.dmol.component_log_probs with the interior mass as the plain difference of two sigmoids (the form the
    kernel and the oracle had before): kept to show that the tail inputs tell the two forms apart."""
    xr, xg = x[:, 0:1], x[:, 1:2]
    m = torch.stack((means[:, 0], means[:, 1] + coeffs[:, 0] * xr,
                     means[:, 2] + coeffs[:, 1] * xr + coeffs[:, 2] * xg), dim=1)
    xx = x.unsqueeze(2)
    centered = xx - m
    inv_s = torch.exp(-log_scales)
    plus_in, min_in, mid_in = inv_s * (centered + BIN), inv_s * (centered - BIN), inv_s * centered
    cdf_delta = torch.sigmoid(plus_in) - torch.sigmoid(min_in)
    log_pdf_mid = mid_in - log_scales - 2.0 * F.softplus(mid_in)
    inner = torch.where(cdf_delta > odmol.MASS_SWITCH, torch.log(cdf_delta.clamp(min=odmol.MASS_FLOOR)),
                        log_pdf_mid - math.log(127.5))
    return torch.where(xx < -0.999, plus_in - F.softplus(plus_in), torch.where(xx > 0.999, -F.softplus(min_in), inner))


def _as_images(rows, x, dtype):
    P = rows.shape[0]
    return rows.to(dtype).t().reshape(1, rows.shape[1], 1, P), x.to(dtype).t().reshape(1, 3, 1, P)


def dmol_ll(rows, x, K, form="stable", dtype=torch.float64):
    """Per-pixel log-likelihood (P,) of rows (P, 10 K), x (P, 3)."""
    l, xx = _as_images(rows, x, dtype)
    if form == "stable":
        return odmol.dmol_log_likelihood(l, xx, K).reshape(-1)
    assert form == "plain"
    logits, means, log_scales, coeffs = odmol.split_params(l, K)
    lp = component_log_probs_plain(xx, means, log_scales, coeffs).sum(dim=1) + F.log_softmax(logits, dim=1)
    return torch.logsumexp(lp, dim=1).reshape(-1)


def dmol_ref(rows, x, K, form="stable", dtype=torch.float64):
    """-> (ll (P,), g (P, 10 K)): g = d(-ll_p) / d rows_p by autograd — the gradient pg_dmol_bwd writes for N = 1 and
    gscale = 1 (pixels are independent, so one backward of the sum gives every pixel's own gradient)."""
    leaf = rows.to(dtype).clone().requires_grad_(True)
    ll = dmol_ll(leaf, x, K, form, dtype)
    (g,) = torch.autograd.grad(-ll.sum(), leaf)
    return ll.detach(), g


def bin_masses(rows, x, K):
    """Float64 bin mass of every INTERIOR sub-pixel under every component, flattened (edge bins have no switch)."""
    l, xx = _as_images(rows, x, torch.float64)
    _, means, log_scales, coeffs = odmol.split_params(l, K)
    h2 = 2.0 * BIN * torch.exp(-log_scales)
    xr, xg = xx[:, 0:1], xx[:, 1:2]
    m = torch.stack((means[:, 0], means[:, 1] + coeffs[:, 0] * xr, means[:, 2] + coeffs[:, 1] * xr + coeffs[:, 2] * xg), 1)
    cen = (xx.unsqueeze(2) - m) * torch.exp(-log_scales)
    log_mass = -F.softplus(-(cen + h2 / 2)) - F.softplus(cen - h2 / 2) + torch.log(-torch.expm1(-h2))
    interior = (xx.unsqueeze(2).abs() <= 0.999).expand_as(log_mass)                # (1, 3, K, 1, P)
    return log_mass[interior].exp()


def ll_excess(got, want):
    """max over pixels of |got - want| / (LL_TOL |want| + LL_ABS): <= 1 passes. Also the worst plain relative error."""
    got, want = got.detach().double().cpu().reshape(-1), want.detach().double().cpu().reshape(-1)
    d = (got - want).abs()
    return float((d / (LL_TOL * want.abs() + LL_ABS)).max()), float((d / want.abs().clamp_min(1e-300)).max())


def assert_ll(got, want, what):
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite log-likelihood"
    ratio, rel = ll_excess(got, want)
    print(f"[heads] {what}: per-pixel ll worst |d| / (1e-4 |want| + {LL_ABS:.1e}) = {ratio:.3e}, worst relative {rel:.3e}")
    assert ratio <= 1.0, f"{what}: per-pixel log-likelihood out of bound, ratio {ratio:.3e} (worst relative {rel:.3e})"


def add_rows(rep, name, got, want):
    """Every ROW of got / want (P, C) is one tensor under _util.GradReport's two bounds (per row: max-norm of the row's
    maximum, and element-wise with the floor at the row's maximum) — vectorised; the report keeps the worst row of each
    kind, named by its index, so that a million rows cost two entries."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape and got.dim() == 2
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite gradient"
    m = want.abs().amax(dim=1)
    # a row whose whole float64 gradient lies below float32's normal range (a saturated edge bin at 100 scales: e^-100)
    # has no float32 digits to compare: there the kernel's row must lie below that range too, and 0 is as good
    tiny = m < F32_TINY
    assert float(got[tiny].abs().max() if bool(tiny.any()) else 0.0) <= F32_TINY, f"{name}: a subnormal row is not"
    got, want, m = got[~tiny], want[~tiny], m[~tiny]
    d = (got - want).abs()
    max_norm = d.amax(dim=1) / m.clamp_min(1e-30)
    elem = (d / (rep.tol * want.abs() + rep.floor * m[:, None]).clamp_min(1e-300)).amax(dim=1)
    for worst in {int(max_norm.argmax()), int(elem.argmax())}:
        rep.rows.append((f"{name}[{worst}]", float(max_norm[worst]), float(elem[worst]), float(m[worst])))


def to_kernel_layout(rows, x, N):
    """P = N * L rows -> l (N, 10 K, L), x (N, 3, L) contiguous, pixel p of sample n = row n * L + p."""
    P, C = rows.shape
    L = P // N
    assert N * L == P
    return rows.reshape(N, L, C).transpose(1, 2).contiguous(), x.reshape(N, L, 3).transpose(1, 2).contiguous()


def from_kernel_layout(dl):
    """(N, 10 K, L) -> rows (N * L, 10 K)."""
    N, C, L = dl.shape
    return dl.transpose(1, 2).reshape(N * L, C)


def mirror(rows, x, K):
    """x -> -x and every mean -> -mean (logits, log-scales, raw coefficients kept): the same likelihood, exactly — the
    negations are exact in float32, the effective means mean_c + coeff * x negate with them, and the values 0 and 255
    swap, so the two edge-bin branches do."""
    out = rows.clone()
    for c in range(3):
        out[:, K + c * 3 * K:K + c * 3 * K + K] *= -1.0
    return out, -x


def mean_sign(K):
    """(10 K,) of -1 on the mean channels and +1 elsewhere: how the gradient of a mirrored row maps back."""
    s = torch.ones(10 * K, dtype=torch.float64)
    for c in range(3):
        s[K + c * 3 * K:K + c * 3 * K + K] = -1.0
    return s


def scale_channels(K):
    return [K + c * 3 * K + K + k for c in range(3) for k in range(K)]


# ---------------------------------------------------------------------------------------------
# DMOL inputs
def pixel(v, comps):
    """One row. v: three 8-bit values; comps: K tuples (logit, t3, s3, a3) — sub-pixel c of the component sits t3[c]
    scales (of exp(max(s3[c], -7))) ABOVE the component's effective mean (negative: below), with log-scale s3[c] and raw
    coefficient a3[c]. Means are worked out in float64 from the float32 pixel and coefficient values, then rounded."""
    K = len(comps)
    x = torch.tensor(v, dtype=torch.float32) / 127.5 - 1.0
    xd = x.double()
    row = torch.zeros(10 * K, dtype=torch.float64)
    for k, (logit, t, s, a) in enumerate(comps):
        row[k] = logit
        c = torch.tanh(torch.tensor(a, dtype=torch.float32).double())
        shift = (0.0, float(c[0] * xd[0]), float(c[1] * xd[0] + c[2] * xd[1]))
        for ch in range(3):
            base = K + ch * 3 * K
            row[base + k] = float(xd[ch]) - t[ch] * math.exp(max(s[ch], odmol.LOG_SCALE_MIN)) - shift[ch]
            row[base + K + k] = s[ch]
            row[base + 2 * K + k] = a[ch]
    return row.float(), x


def _stack(pixels):
    return torch.stack([p[0] for p in pixels]), torch.stack([p[1] for p in pixels])


A_DEFAULT = (0.3, -0.5, 0.7)
A_ZERO = (0.0, 0.0, 0.0)
V_INTERIOR = (100, 37, 200)


def tail_sweep():
    """K = 1, interior pixel. Row ((i_s * 13 + i_t) * 2 + sign) for the grid S_SWEEP x T_SWEEP x {above, below} with all
    three sub-pixels at t; then S_SWEEP x T_MIXED x {above, below}. Even rows are the upper tail, the next row its mirror
    image in t. The raw coefficients are 0 here (the other families couple the sub-pixels): the effective means are then
    the stored ones and x - mean is exact in float32, so that t = 0 and 0.3 at scales of e^-7 are what they say — with a
    coupling, the rounding of mean + coeff * x (3e-8) is 3e-5 scales there, and the gradient at the mode, which is that
    offset times the curvature, would be all rounding. -> (rows, x, K, labels)."""
    pixels, labels = [], []
    for s in S_SWEEP:
        for t in T_SWEEP:
            for sign in (1.0, -1.0):
                pixels.append(pixel(V_INTERIOR, [(0.0, (sign * t,) * 3, (s,) * 3, A_ZERO)]))
                labels.append((s, t, sign))
    for s in S_SWEEP:
        for t3 in T_MIXED:
            for sign in (1.0, -1.0):
                pixels.append(pixel(V_INTERIOR, [(0.0, tuple(sign * t for t in t3), (s,) * 3, A_ZERO)]))
                labels.append((s, t3, sign))
    return _stack(pixels) + (1, labels)


def branch_cases():
    """K = 1, one row per branch of subpixel(): -> (rows, x, K, labels)."""
    cases = []

    def add(label, v, t, s, a=A_DEFAULT):
        t = t if isinstance(t, tuple) else (t,) * 3
        s = s if isinstance(s, tuple) else (s,) * 3
        cases.append((label, pixel(v, [(0.0, t, s, a)])))

    for t in (60.0, -60.0, 100.0, -100.0, 0.4, -3.0):           # value 0 / 255: log sigmoid(pin), log(1 - sigmoid(nin))
        add(f"value 0, t={t}", (0, 0, 0), t, -3.0)
        add(f"value 255, t={t}", (255, 255, 255), t, -3.0)
    add("values 0 / 255 / interior", (0, 255, 128), (-60.0, 60.0, 1.0), -3.0)
    add("values 255 / 0 / interior", (255, 0, 90), (2.0, -2.0, -1.0), (-1.0, -5.0, 0.5))
    for s in (-3.0, 0.5, -6.5):                                  # values 1 and 254 are interior bins
        for t in (2.0, -2.0):
            add(f"values 1 / 254 / 1, s={s}, t={t}", (1, 254, 1), t, s)
            add(f"values 254 / 1 / 254, s={s}, t={t}", (254, 1, 254), t, s)
    for s, t in ((-2.0, 30.0), (0.5, 8.0), (-5.0, 20.0)):        # density fallback, either tail
        add(f"fallback s={s} t={t}", V_INTERIOR, t, s)
        add(f"fallback s={s} t={-t}", V_INTERIOR, -t, s)
    for s in (-6.999, -7.001, -7.5, -20.0):                      # either side of the clamp (never -7.0 itself)
        for t in (1.0, -1.0, 14.0):
            add(f"clamp s={s} t={t}", V_INTERIOR, t, s)
    add("clamp, one sub-pixel only", V_INTERIOR, (1.0, -2.0, 0.5), (-3.0, -8.0, -6.0))
    for vr, a in ((0, (8.0, 8.0, 8.0)), (255, (8.0, -8.0, 8.0)), (0, (-8.0, 8.0, -8.0)), (255, (-8.0, -8.0, -8.0))):
        add(f"coefficients {a}, x_r from value {vr}", (vr, 128, 60), (0.5, -1.0, 1.5), -2.0, a)
        add(f"coefficients {a}, x_r = x_g from value {vr}", (vr, vr, 60), (0.5, -1.0, 1.5), -2.0, a)
    labels = [c[0] for c in cases]
    return _stack([c[1] for c in cases]) + (1, labels)


_V_CYCLE = ((100, 37, 200), (0, 128, 255), (1, 254, 77), (255, 0, 13))


def _random_comp(g, t_max=3.0):
    u = torch.rand(9, generator=g).tolist()
    return (float(torch.randn(1, generator=g)) * 2.0, tuple((2 * u[i] - 1) * t_max for i in range(3)),
            tuple(-4.0 + 4.5 * u[3 + i] for i in range(3)), tuple(3.0 * (2 * u[6 + i] - 1) for i in range(3)))


def mixture_cases(K):
    """-> (rows, x, K, labels) for one K of MIXTURE_KS."""
    g = _gen(K, 31)
    cases = []
    for i, v in enumerate(_V_CYCLE):
        cases.append((f"random {i}", pixel(v, [_random_comp(g) for _ in range(K)])))
    for i, v in enumerate(_V_CYCLE[:2]):
        comps = [_random_comp(g) for _ in range(K)]
        cases.append((f"logits +-60 {i}", pixel(v, [((60.0 if (k + i) % 2 == 0 else -60.0),) + c[1:]
                                                    for k, c in enumerate(comps)])))
        comps = [_random_comp(g) for _ in range(K)]
        comps[K - 1] = (-1.0e4,) + comps[K - 1][1:]
        cases.append((f"one logit -1e4 {i}", pixel(v, comps)))
    # every component far from the pixel: fallback branch, mid - s - 2 softplus(mid) - log 127.5 ~ -64 + 2 - 4.85 per
    # sub-pixel, so every joint log-probability is about -200
    far = [(0.1 * k, tuple((64.0 if (k + c) % 2 else -64.0) + 0.05 * k for c in range(3)), (-2.0,) * 3, A_DEFAULT)
           for k in range(K)]
    cases.append(("all components at -200", pixel(V_INTERIOR, far)))
    for exact in sorted({0, K - 1}):
        comps = [(0.2 * k, ((40.0 if k % 2 else -40.0),) * 3, (-3.0,) * 3, A_DEFAULT) for k in range(K)]
        comps[exact] = (-0.5, (0.1, -0.2, 0.05), (-4.0,) * 3, (1.0, -1.0, 0.5))
        cases.append((f"component {exact} exact, the rest negligible", pixel(V_INTERIOR, comps)))
    labels = [c[0] for c in cases]
    return _stack([c[1] for c in cases]) + (K, labels)


def dmol_families():
    """name -> (rows, x, K, labels): every DMOL input of the GPU tier (the indexing cases draw their pixels from these)."""
    fams = {"tail": tail_sweep(), "branch": branch_cases()}
    for K in MIXTURE_KS:
        fams[f"mix{K}"] = mixture_cases(K)
    return fams


INDEX_L = (1, 63, 64, 65, 255, 257)
INDEX_N = (1, 3)
GRID_STRIDE_NL = (3, 349527)      # N * L = 1048581 > 4096 * 256 = 1048576: the forward's 2048 blocks and the
#                                   backward's 4096 both go round their grid-stride loop


def index_pool(K):
    """The rows the indexing cases are assembled from: K = 1 -> tail sweep + branches, K = 3 -> the K = 3 mixtures."""
    if K == 1:
        a, b = tail_sweep(), branch_cases()
        return torch.cat([a[0], b[0]]), torch.cat([a[1], b[1]])
    rows, x, _, _ = mixture_cases(K)
    return rows, x


def index_pick(P, pool_size, salt=0):
    """Which pool row pixel i of an indexing case is: neighbours differ, and no period divides a block or a row."""
    return (torch.arange(P, dtype=torch.int64) * 7919 + salt) % pool_size


# ---------------------------------------------------------------------------------------------
# Gaussian heads: the three formulas of csrc/vae_ops.hip / include/pg_hip.h
def gauss_head(q, p, eps, C, mode, dtype=torch.float64):
    """q, p: (N, >= 2 C, L) with [mean | log_std] in the first 2 C channels (q is None in mode 2, p in mode 0); eps
    (N, C, L). -> (z (N, C, L), kl (N,) or None):
      mode 0: z = mu_q + exp(s_q) eps,  kl[n] = sum -0.5 (1 + 2 s_q - exp(2 s_q) - mu_q^2)
      mode 1: same z,                   kl[n] = sum -0.5 + (s_p - s_q) + (exp(2 s_q) + (mu_q - mu_p)^2) / (2 exp(2 s_p))
      mode 2: z = mu_p + exp(s_p) eps,  no kl."""
    e = eps.to(dtype)
    if mode == 2:
        p = p.to(dtype)
        return p[:, :C] + torch.exp(p[:, C:2 * C]) * e, None
    q = q.to(dtype)
    mq, sq = q[:, :C], q[:, C:2 * C]
    z = mq + torch.exp(sq) * e
    if mode == 0:
        kl = -0.5 * (1.0 + 2.0 * sq - torch.exp(2.0 * sq) - mq * mq)
    else:
        p = p.to(dtype)
        mp, sp = p[:, :C], p[:, C:2 * C]
        # the quotient of the header written as a product with exp(-2 s_p): the same number, and a float32 autograd of
        # it does not square the denominator (which overflows for s_p = -20 although no gradient does)
        kl = -0.5 + (sp - sq) + 0.5 * (torch.exp(2.0 * sq) + (mq - mp) ** 2) * torch.exp(-2.0 * sp)
    return z, kl.sum(dim=(1, 2))


def gauss_head_ref(q, p, eps, C, mode, dz, dkl, dtype=torch.float64):
    """Forward and the gradients pg_gauss_head_bwd writes (autograd of sum(z dz) + sum(kl dkl); dz / dkl None = 0).
    -> (z, kl, dq (N, 2 C, L) or None, dp (N, 2 C, L) or None)."""
    ql = None if q is None or mode == 2 else q[:, :2 * C].to(dtype).clone().requires_grad_(True)
    pl = None if p is None or mode == 0 else p[:, :2 * C].to(dtype).clone().requires_grad_(True)
    z, kl = gauss_head(ql, pl, eps, C, mode, dtype)
    obj = z.sum() * 0.0
    if dz is not None:
        obj = obj + (z * dz.to(dtype)).sum()
    if dkl is not None and kl is not None:
        obj = obj + (kl * dkl.to(dtype)).sum()
    leaves = [t for t in (ql, pl) if t is not None]
    grads = list(torch.autograd.grad(obj, leaves, allow_unused=True))
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, leaves)]
    dq = grads.pop(0) if ql is not None else None
    dp = grads.pop(0) if pl is not None else None
    return z.detach(), None if kl is None else kl.detach(), dq, dp


GAUSS_CL = {1: (1, 1), 63: (3, 21), 64: (4, 16), 255: (5, 51), 256: (4, 64), 257: (1, 257), 16384: (16, 1024),
            16385: (5, 3277), 40000: (10, 4000)}   # C * L -> (C, L); 16384 = 64 blocks of 256 exactly, beyond it they loop
GAUSS_N = (1, 3)
GAUSS_EXTRA = (0, 5)              # channels beyond [mean | log_std] (VD-VAE's prior carries more)
# Log-stds beyond about 44 overflow exp(2 s) in float32 (e^88 ~ 1.7e38), and a pair (s_q, s_p) overflows the ratio
# exp(2 s_q) / exp(2 s_p) from s_q - s_p ~ 44: +-20 is as far as a pair may go, and nothing here goes further.
GAUSS_PAIRS = ((20.0, 20.0), (-20.0, -20.0), (20.0, -20.0), (-20.0, 20.0), (20.0, 0.0), (0.0, -20.0))


def gauss_inputs(C, L, N, q_extra, p_extra, regime, seed=0):
    """q (N, 2 C + q_extra, L), p (N, 2 C + p_extra, L), eps, dz (N, C, L), dkl (N,) — float32.
    regime "moderate": means and log-stds ~ 0.5 N(0, 1) (what the model tests feed); "wide": log-stds uniform over
    [-8, 8], means uniform over [-30, 30]. The extra channels hold values a kernel reading them as log-stds would
    overflow on (60)."""
    g = _gen(C, L, N, q_extra, p_extra, seed, regime == "wide")
    out = []
    for extra in (q_extra, p_extra):
        t = torch.full((N, 2 * C + extra, L), 60.0)
        if regime == "moderate":
            t[:, :2 * C] = 0.5 * torch.randn(N, 2 * C, L, generator=g)
        else:
            t[:, :C] = 60.0 * torch.rand(N, C, L, generator=g) - 30.0
            t[:, C:2 * C] = 16.0 * torch.rand(N, C, L, generator=g) - 8.0
        out.append(t)
    eps = torch.randn(N, C, L, generator=g)
    dz = torch.randn(N, C, L, generator=g)
    dkl = torch.randn(N, generator=g)
    return out[0], out[1], eps, dz, dkl


def gauss_pair_inputs():
    """One element per sample (C = L = 1), sample n = pair n of GAUSS_PAIRS as (s_q, s_p), means +-30 apart."""
    N = len(GAUSS_PAIRS)
    q, p = torch.zeros(N, 2, 1), torch.zeros(N, 2, 1)
    for n, (sq, sp) in enumerate(GAUSS_PAIRS):
        q[n, 0, 0], q[n, 1, 0] = 30.0 if n % 2 else -30.0, sq
        p[n, 0, 0], p[n, 1, 0] = -q[n, 0, 0], sp
    g = _gen(N, 77)
    return q, p, torch.randn(N, 1, 1, generator=g), torch.randn(N, 1, 1, generator=g), torch.randn(N, generator=g)


VEC_MEAN_N = (1, 63, 64, 65, 1000)
FILL_N = (1, 255, 256, 257, 16385)


def vec_mean_inputs(n):
    return torch.randn(n, generator=_gen(n, 5)) + 0.25

