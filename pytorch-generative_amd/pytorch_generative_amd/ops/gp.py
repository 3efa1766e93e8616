"""ops.gp — the dense symmetric solve of a Gaussian process on the kernels of csrc/gp.hip: squared-exponential covariance, a
blocked fp32 Cholesky factorisation that can be appended to, the triangular solves X L^T = B and X L = B, and the strided GEMM
update C = C -/+ A B^T. Every operand is a 2-D fp32 tensor whose rows are contiguous and whose row stride may be larger than
its row (a view of a larger buffer is an operand as it lies). Functions ending in an underscore work in place. No gradients.
The second half works on csrc/gp_mll.hip: the triangular inverse of a factor, the product that turns it into K^-1, and the
reductions that give the log marginal likelihood and its gradients with respect to the hyperparameters as numbers on the device.
The third part serves the stationary kernels beyond the shared-lengthscale squared exponential: Matern 3/2 and 5/2, and one
lengthscale per input column (ARD) for all three kinds, with the reduction that gives every d/d lengthscale_c.

Part of the operator layer (pytorch_generative_amd.ops): HIP kernels called through the C-ABI with tensor.data_ptr() and the
current stream. No CPU / ATen fallback: a missing library, a CPU tensor or a shape outside ops.gp_plan raises."""

import ctypes

import torch

from pytorch_generative_amd import _lib
from pytorch_generative_amd.ops._common import _chk, _stream

GP_PLAN_INTS = 16  # PG_GP_PLAN_INTS
GP_LOWER, GP_MIRROR, GP_DIAG, GP_PLUS, GP_B_TRANS, GP_SE_DIRECT, GP_SE_MFMA = 1, 2, 4, 8, 16, 32, 64  # PG_GP_*
_PLAN_FIELDS = ("tile", "k_chunk", "panels", "row_tiles", "se_route", "se_direct_max_d", "se_symmetric_tiles", "se_cross_tiles",
                "potrf_launches", "trsm_launches", "trailing_workgroups", "max_n", "max_d", "max_p", "p_row_tiles",
                "se_direct_forced_max_d")
_SE_ROUTES = {None: 0, "direct": GP_SE_DIRECT, "mfma": GP_SE_MFMA}


def _plan_status(entry, ints, fields, *dims):
    """(status, plan) of the host-only planner `entry`: its C-ABI status (0, PG_ESHAPE = -2, PG_EINVAL = -1) and the plan dict
    (None on error)."""
    out = (ctypes.c_longlong * ints)()
    rc = getattr(_lib.load(), entry)(*map(int, dims), out, ints)
    return rc, (None if rc else dict(zip(fields, out)))


def gp_plan_status(n, m, d, p):
    """(status, plan) of pg_gp_plan, see _plan_status."""
    return _plan_status("pg_gp_plan", GP_PLAN_INTS, _PLAN_FIELDS, n, m, d, p)


def gp_plan(n, m, d, p):
    """The planner's answer (pg_gp_plan, host only) for n training rows, m query rows, d input columns and p columns of y: None
    for a problem it refuses (n, m in 1 .. 16384, d, p in 1 .. 4096), else a dict with the panel width, the k chunk, the panels
    of n, the row tiles of m, the covariance route (0: exact differences, 1: the MFMA) and the largest d of route 0, the tiles
    of the symmetric and the cross covariance, the launches of a full factorisation and of a forward solve, the workgroups of
    the first trailing update, the domain's edges, the row tiles of p and the largest d route 0 takes when forced."""
    return gp_plan_status(n, m, d, p)[1]


def _mat(t, name):
    """A 2-D fp32 matrix on the current GPU with contiguous rows; returns (tensor, row stride). Never copies."""
    if t.dim() != 2:
        raise ValueError(f"{name}: expected a 2-D matrix, got shape {tuple(t.shape)}")
    if t.requires_grad:
        raise ValueError(f"{name}: the Gaussian-process operators build no gradients (requires_grad is set)")
    if t.numel() == 0:
        raise ValueError(f"{name}: empty matrix of shape {tuple(t.shape)}")
    _chk(t[:1, :1], name)  # the device and dtype checks of every family, on a view that is never copied
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise ValueError(f"{name}: rows must be contiguous (strides {t.stride()})")
    ld = t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0))
    if ld < t.shape[1]:
        raise ValueError(f"{name}: row stride {ld} below the row length {t.shape[1]}")
    return t, ld


def se_kernel(a, b, std, lengthscale, noise_var=0.0, *, out=None, mirror=True, diag_offset=None, route=None):
    """The squared-exponential covariance K[i, j] = std^2 exp(-|a_i - b_j|^2 / (2 lengthscale^2)) of a (n, d) and b (m, d),
    (n, m), into `out` if given (any row stride).

    `b is a`: the symmetric form. Only the tiles on or below the diagonal are computed, the diagonal is exactly
    std^2 + noise_var, and with mirror=True (default) the lower triangle is copied into the upper one, so the result is exactly
    symmetric; with mirror=False the strict upper triangle of `out` above the diagonal tiles is left as it was.
    diag_offset = o (cross form): only the elements j <= i + o are written and the elements j == i + o are exactly
    std^2 + noise_var — rows of a larger symmetric matrix. Otherwise every element is written and noise_var is not used.
    route: None (ops.gp_plan decides: exact differences for d <= 16, |a|^2 + |b|^2 - 2 a.b on the MFMA above), "direct"
    (d <= 64) or "mfma". One launch, capturable, bit-identical from run to run; an element depends on its two rows alone.
    stationary_kernel with kind "se" under this function's name."""
    return _stationary_kernel("se_kernel", a, b, std, float(lengthscale), noise_var, "se", out, mirror, diag_offset, route, None)


def add_diag_(a, value):
    """a[i, i] += value for the square matrix a, in place; returns a."""
    a, ld = _mat(a, "add_diag_.a")
    if a.shape[0] != a.shape[1]:
        raise ValueError(f"add_diag_: expected a square matrix, got {tuple(a.shape)}")
    _lib.check(_lib.load().pg_gp_add_diag(a.data_ptr(), ld, a.shape[0], float(value), _stream()), "pg_gp_add_diag")
    return a


def gemm_nt_(c, a, b, *, add=False, lower=False, mirror=False, b_transposed=False, diag_offset=0):
    """c (R, C) -= a b^T in place (add=True: +=) for a (R, K) and b (C, K); b_transposed: b is (K, C), the a b form. Returns c.

    The accumulators are seeded with c and the product is subtracted inside the fp32-MFMA chain: each element is
    fmaf(-a_k, b_k, .) in ascending k starting from c's value, so an update applied in pieces along k has the bits of the
    update applied at once. lower: only the elements col <= row + diag_offset are read and written; mirror (square, lower,
    diag_offset 0): c[col, row] = c[row, col] as well. One launch, capturable, bit-identical from run to run."""
    c, ldc = _mat(c, "gemm_nt_.c")
    a, lda = _mat(a, "gemm_nt_.a")
    b, ldb = _mat(b, "gemm_nt_.b")
    r, cc = c.shape
    k = a.shape[1]
    want_b = (k, cc) if b_transposed else (cc, k)
    if a.shape[0] != r or tuple(b.shape) != want_b:
        raise ValueError(f"gemm_nt_: c {tuple(c.shape)}, a {tuple(a.shape)}, b {tuple(b.shape)} do not fit (b should be {want_b})")
    flags = (GP_PLUS if add else 0) | (GP_LOWER if lower else 0) | (GP_MIRROR if mirror else 0) | (GP_B_TRANS if b_transposed else 0)
    _lib.check(_lib.load().pg_gp_gemm_nt(a.data_ptr(), lda, b.data_ptr(), ldb, c.data_ptr(), ldc, r, cc, k, int(diag_offset), flags,
                                         _stream()), "pg_gp_gemm_nt")
    return c


def _info(info, device):
    if info is None:
        return torch.zeros(1, dtype=torch.int32, device=device)
    if not info.is_cuda or info.dtype != torch.int32 or info.numel() != 1:
        raise ValueError("cholesky_: info must be one int32 on the GPU")
    return info


def cholesky_(a, n_done=0, info=None):
    """The lower Cholesky factor of the symmetric positive definite a (n, n), in place in its lower triangle; the strict upper
    triangle is neither read nor written. Returns info, one int32 on the GPU (a given `info` is used as it is and must be 0):
    0, or index + 1 of the first pivot that was not > 0 — the launches return normally then and the factor holds NaNs. Reading
    info is the caller's host synchronisation.

    n_done > 0: rows < n_done already hold the factor of the leading (n_done, n_done) block and rows n_done .. n hold a's
    values (columns 0 .. their own); only those rows are completed, and the result has the bits of the full factorisation.
    Blocked, right-looking, at most three launches per panel of 64 columns (ops.gp_plan), capturable."""
    a, ld = _mat(a, "cholesky_.a")
    if a.shape[0] != a.shape[1]:
        raise ValueError(f"cholesky_: expected a square matrix, got {tuple(a.shape)}")
    info = _info(info, a.device)
    _lib.check(_lib.load().pg_gp_potrf(a.data_ptr(), ld, a.shape[0], int(n_done), info.data_ptr(), _stream()), "pg_gp_potrf")
    return info


def trsm_right_(l, x, col_done=0, transposed=False):
    """Solves x l^T = b (transposed=True: x l = b) in place for the lower-triangular l (n, n) — its strict upper triangle is
    not read — and x (rows, n) holding b; returns x. col_done > 0 (forward form only): columns < col_done of x are final and
    only the others, which hold b, are completed, with the bits of the full solve. Right-looking, two launches per panel of 64
    columns, capturable."""
    l, ld = _mat(l, "trsm_right_.l")
    x, ldx = _mat(x, "trsm_right_.x")
    if l.shape[0] != l.shape[1] or x.shape[1] != l.shape[0]:
        raise ValueError(f"trsm_right_: l {tuple(l.shape)} and x {tuple(x.shape)} do not fit")
    _lib.check(_lib.load().pg_gp_trsm_right(l.data_ptr(), ld, l.shape[0], x.data_ptr(), ldx, x.shape[0], int(col_done),
                                            int(bool(transposed)), _stream()), "pg_gp_trsm_right")
    return x


# ---------------------------------------------------------------------------------------------
# the log marginal likelihood and its hyperparameter gradients (csrc/gp_mll.hip)
GP_MLL_PLAN_INTS = 16  # PG_GP_MLL_PLAN_INTS
_MLL_PLAN_FIELDS = ("tile", "panels", "inverse_launches", "inverse_tile_products", "gram_tiles", "gram_tile_products", "sums_tiles",
                    "sums_partial_rows", "workspace_floats", "se_route", "se_direct_max_d", "max_n", "max_d", "max_p", "outer_k_chunks",
                    "sums_launches")


def gp_mll_plan_status(n, d, p):
    """(status, plan) of pg_gp_mll_plan, see _plan_status."""
    return _plan_status("pg_gp_mll_plan", GP_MLL_PLAN_INTS, _MLL_PLAN_FIELDS, n, d, p)


def gp_mll_plan(n, d, p):
    """The planner's answer (pg_gp_mll_plan, host only) for the marginal likelihood of n training rows with d input columns and p
    columns of y: None for a problem it refuses (the domain of gp_plan), else a dict with the tile edge, the panels of n, the
    launches and the 64x64x64 tile-products of the triangular inverse, the tiles and the tile-products of X X^T, the tiles and
    the partial rows of the reduction, the workspace floats se_mll_sums needs, the covariance route of the reduction (as
    se_kernel's) and its threshold, the domain's edges, the k chunks of the in-kernel outer product (every p takes that route)
    and the launches of the reduction."""
    return gp_mll_plan_status(n, d, p)[1]


def _vec(t, size, name, at_least=False):
    """A contiguous 1-D fp32 vector of `size` elements (or more, with at_least) on the current GPU."""
    if t.dim() != 1 or (t.numel() < size if at_least else t.numel() != size):
        raise ValueError(f"{name}: expected a 1-D tensor of {'at least ' if at_least else ''}{size} floats, got shape {tuple(t.shape)}")
    if t.requires_grad:
        raise ValueError(f"{name}: the Gaussian-process operators build no gradients (requires_grad is set)")
    _chk(t[:1], name)
    if t.numel() > 1 and t.stride(0) != 1:
        raise ValueError(f"{name}: must be contiguous (stride {t.stride(0)})")
    return t


def _square(t, name):
    t, ld = _mat(t, name)
    if t.shape[0] != t.shape[1]:
        raise ValueError(f"{name}: expected a square matrix, got {tuple(t.shape)}")
    return t, ld


def tri_inverse_t(l, out=None):
    """X = l^-T for the lower-triangular l (n, n), into the UPPER triangle of `out` (diagonal included; any row stride), which is
    returned. The strict lower triangle of `out` and the strict upper triangle of l are neither read nor written; without `out`
    a zeroed matrix is made, so the result is the triangular matrix itself. The right-looking solve of X l^T = I in panels of
    64 columns, restricted to the rows above each panel's end (the others are zero): about n^3 / 3 flops, 2 panels - 1
    launches (ops.gp_mll_plan), capturable, bit-identical from run to run."""
    l, ld = _square(l, "tri_inverse_t.l")
    n = l.shape[0]
    if out is None:
        out = torch.zeros((n, n), device=l.device, dtype=torch.float32)
    out, ldx = _square(out, "tri_inverse_t.out")
    if out.shape[0] != n:
        raise ValueError(f"tri_inverse_t: out of shape {tuple(out.shape)}, expected {(n, n)}")
    _lib.check(_lib.load().pg_gp_trtri_t(l.data_ptr(), ld, n, out.data_ptr(), ldx, _stream()), "pg_gp_trtri_t")
    return out


def gram_upper_(h, x, *, mirror=False):
    """h = x x^T for the UPPER-triangular x (n, n) — its strict lower triangle is not read — on the lower triangle of h (n, n),
    diagonal included, in place; mirror=True writes h[j, i] = h[i, j] as well. Returns h. Only the tiles on or below the
    diagonal are visited and tile (I, J) starts its k loop at row tile I, where x's rows begin: about n^3 / 3 flops. Each
    element is one fmaf chain in ascending k (no k-split). One launch, capturable, bit-identical from run to run."""
    h, ldh = _square(h, "gram_upper_.h")
    x, ldx = _square(x, "gram_upper_.x")
    if h.shape[0] != x.shape[0]:
        raise ValueError(f"gram_upper_: h {tuple(h.shape)} and x {tuple(x.shape)} do not fit")
    _lib.check(_lib.load().pg_gp_gram_upper(x.data_ptr(), ldx, x.shape[0], h.data_ptr(), ldh, GP_MIRROR if mirror else 0, _stream()),
               "pg_gp_gram_upper")
    return h


def se_mll_sums(x, std, lengthscale, h, alpha_t, *, out=None, workspace=None):
    """The contraction of G = alpha alpha^T - p h with the squared-exponential covariance K_f of the rows of x (n, d) and its
    derivatives, for h (n, n) = K^-1 (only its lower triangle is read) and alpha_t (p, n): the 1-D tensor
        (sum_ij G_ij K_f,ij / std,  sum_ij G_ij K_f,ij |x_i - x_j|^2 / (2 lengthscale^3),  tr G / 2)
    on the GPU, into `out` (3 floats) if given — the gradients of the log marginal likelihood with respect to std, lengthscale
    and noise_var. One workgroup per 64 x 64 tile on or below the diagonal recomputes the distances (se_kernel's routes and
    bits), so neither K_f, its derivative nor G is written to memory; `workspace` (ops.gp_mll_plan's workspace_floats, made if
    not given) takes one fp32 partial row per tile, which a second launch adds in double in a fixed order. No atomics:
    bit-identical from run to run. Two launches, capturable. stationary_mll_sums with kind "se" under this function's name."""
    return _stationary_mll_sums("se_mll_sums", x, std, lengthscale, h, alpha_t, "se", out, workspace)


def mll_value(l, zt, alpha_t, *, out=None):
    """(log p(y), sum alpha) as a 1-D tensor of 2 floats on the GPU (into `out` if given) from the lower factor l (n, n) of the
    training covariance, zt (p, n) = (l^-1 r)^T and alpha_t (p, n) = (l^-T l^-1 r)^T:
    log p(y) = -1/2 sum zt^2 - p sum_i log l_ii - (n p / 2) log 2 pi. One workgroup, double accumulators, a fixed order."""
    l, ld = _square(l, "mll_value.l")
    zt, ldz = _mat(zt, "mll_value.zt")
    alpha_t, lda = _mat(alpha_t, "mll_value.alpha_t")
    n = l.shape[0]
    p = zt.shape[0]
    if zt.shape[1] != n or tuple(alpha_t.shape) != (p, n):
        raise ValueError(f"mll_value: l {tuple(l.shape)}, zt {tuple(zt.shape)} and alpha_t {tuple(alpha_t.shape)} do not fit")
    if out is None:
        out = torch.empty(2, device=l.device, dtype=torch.float32)
    out = _vec(out, 2, "mll_value.out")
    _lib.check(_lib.load().pg_gp_mll_value(l.data_ptr(), ld, n, zt.data_ptr(), ldz, alpha_t.data_ptr(), lda, p, out.data_ptr(), _stream()),
               "pg_gp_mll_value")
    return out


# ---------------------------------------------------------------------------------------------
# stationary kernels with per-dimension (ARD) lengthscales: squared exponential, Matern 3/2 and 5/2
GP_ARD_PLAN_INTS = 8  # PG_GP_ARD_PLAN_INTS
GP_KINDS = {"se": 0, "matern32": 1, "matern52": 2}  # PG_GP_KIND_*
_ARD_PLAN_FIELDS = ("tile", "sums_tiles", "partial_row_floats", "workspace_floats", "column_chunks", "sums_launches", "max_d", "chunk_columns")


def gp_ard_plan_status(n, d, p):
    """(status, plan) of pg_gp_ard_plan, see _plan_status."""
    return _plan_status("pg_gp_ard_plan", GP_ARD_PLAN_INTS, _ARD_PLAN_FIELDS, n, d, p)


def gp_ard_plan(n, d, p):
    """The planner's answer (pg_gp_ard_plan, host only) for the per-dimension lengthscale gradients of n training rows with d
    input columns and p columns of y: None for a problem it refuses (the domain of gp_mll_plan, and d <= 256), else a dict with
    the tile edge, the tiles (= partial rows) of the reduction, the floats of a partial row (d + 2), the workspace floats
    ard_mll_sums needs, the column chunks the rows of x are staged in, the launches, the largest d and the columns of a chunk."""
    return gp_ard_plan_status(n, d, p)[1]


def _kind(kind, name):
    if kind not in GP_KINDS:
        raise ValueError(f"{name}: kind {kind!r} is none of {sorted(GP_KINDS)}")
    return GP_KINDS[kind]


def _lengthscale(lengthscale, inv_lengthscale, d, name):
    """(the scalar lengthscale for the C-ABI, the device vector 1 / lengthscale or None). A tensor lengthscale is per dimension;
    inv_lengthscale is the caller's cached reciprocal of it, which is then not computed again."""
    if inv_lengthscale is None and not torch.is_tensor(lengthscale):
        return float(lengthscale), None
    given = lengthscale if inv_lengthscale is None else inv_lengthscale
    if given.dim() != 1 or given.numel() != d:
        raise ValueError(f"{name}: a per-dimension lengthscale of shape {tuple(given.shape)} for inputs of {d} columns")
    given = _vec(given, d, f"{name}.lengthscale")
    return 1.0, (given.reciprocal() if inv_lengthscale is None else given)


def stationary_kernel(a, b, std, lengthscale, noise_var=0.0, *, kind="se", out=None, mirror=True, diag_offset=None, route=None,
                      inv_lengthscale=None):
    """The stationary covariance K[i, j] = std^2 phi(r_ij) of a (n, d) and b (m, d), (n, m), r^2 = sum_c ((a_ic - b_jc) / l_c)^2:
    kind "se" (phi = exp(-r^2 / 2)), "matern32" ((1 + sqrt(3) r) exp(-sqrt(3) r)) or "matern52"
    ((1 + sqrt(5) r + 5 r^2 / 3) exp(-sqrt(5) r)). lengthscale: a float (shared) or a 1-D fp32 tensor of d entries on the GPU
    (one per input column); inv_lengthscale: its reciprocal, if the caller keeps one (lengthscale is then not read).

    `b is a`, mirror, diag_offset, out and route are se_kernel's, with the same promises: the diagonal exactly std^2 + noise_var,
    exact symmetry, an element's bits depending on its two rows and the lengthscales alone. The exact-difference route
    (d <= 16, forced up to 64) scales the DIFFERENCE, so inputs far from the origin lose nothing and a duplicated row gives
    exactly std^2; the MFMA route scales the rows while staging them. kind "se" with a float lengthscale is se_kernel. One
    launch, capturable, bit-identical from run to run."""
    return _stationary_kernel("stationary_kernel", a, b, std, lengthscale, noise_var, kind, out, mirror, diag_offset, route, inv_lengthscale)


def _stationary_kernel(name, a, b, std, lengthscale, noise_var, kind, out, mirror, diag_offset, route, inv_lengthscale):
    """stationary_kernel, and se_kernel with kind "se", under the `name` their messages carry."""
    a, lda = _mat(a, f"{name}.a")
    sym = b is a
    b, ldb = (a, lda) if sym else _mat(b, f"{name}.b")
    n, d = a.shape
    m = b.shape[0]
    if b.shape[1] != d:
        raise ValueError(f"{name}: a has {d} columns, b {b.shape[1]}")
    if route not in _SE_ROUTES:
        raise ValueError(f"{name}: route {route!r} is none of None, 'direct', 'mfma'")
    code = _kind(kind, name)
    scalar, inv = _lengthscale(lengthscale, inv_lengthscale, d, name)
    rc, _ = gp_plan_status(n, m, d, 1)
    _lib.check(rc, name)
    if out is None:
        out = torch.empty((n, m), device=a.device, dtype=torch.float32)
    out, ldk = _mat(out, f"{name}.out")
    if tuple(out.shape) != (n, m):
        raise ValueError(f"{name}: out of shape {tuple(out.shape)}, expected {(n, m)}")
    flags = _SE_ROUTES[route]
    off = 0
    if sym:
        if diag_offset is not None:
            raise ValueError(f"{name}: diag_offset belongs to the cross form")
        flags |= GP_LOWER | GP_DIAG | (GP_MIRROR if mirror else 0)
    elif diag_offset is not None:
        flags |= GP_LOWER | GP_DIAG
        off = int(diag_offset)
    _lib.check(_lib.load().pg_gp_stat_kernel(code, a.data_ptr(), lda, n, b.data_ptr(), ldb, m, d, float(std), scalar,
                                             None if inv is None else inv.data_ptr(), float(noise_var), out.data_ptr(), ldk, off, flags,
                                             _stream()), "pg_gp_stat_kernel")
    return out


def _sums_operands(x, h, alpha_t, name):
    x, ldx = _mat(x, f"{name}.x")
    h, ldh = _square(h, f"{name}.h")
    alpha_t, lda = _mat(alpha_t, f"{name}.alpha_t")
    if h.shape[0] != x.shape[0] or alpha_t.shape[1] != x.shape[0]:
        raise ValueError(f"{name}: x {tuple(x.shape)}, h {tuple(h.shape)} and alpha_t {tuple(alpha_t.shape)} do not fit")
    return x, ldx, h, ldh, alpha_t, lda


def _sums_buffers(workspace, out, plan, out_floats, device, name):
    """The workspace (at least the plan's workspace_floats) and `out` (out_floats) of a reduction: made if None, else checked."""
    if workspace is None:
        workspace = torch.empty(plan["workspace_floats"], device=device, dtype=torch.float32)
    workspace = _vec(workspace, plan["workspace_floats"], f"{name}.workspace", at_least=True)
    if out is None:
        out = torch.empty(out_floats, device=device, dtype=torch.float32)
    return workspace, _vec(out, out_floats, f"{name}.out")


def stationary_mll_sums(x, std, lengthscale, h, alpha_t, *, kind="se", out=None, workspace=None):
    """se_mll_sums for any kind of stationary_kernel with one shared lengthscale (a float): the 1-D tensor
        (sum_ij G_ij K_f,ij / std,  sum_ij G_ij std^2 omega(r_ij) r_ij^2 / (2 lengthscale),  tr G / 2),   omega = -phi'(r) / r,
    the gradients of the log marginal likelihood with respect to std, lengthscale and noise_var. Same operands, workspace
    (ops.gp_mll_plan) and promises; kind "se" is se_mll_sums. Two launches, capturable."""
    return _stationary_mll_sums("stationary_mll_sums", x, std, lengthscale, h, alpha_t, kind, out, workspace)


def _stationary_mll_sums(name, x, std, lengthscale, h, alpha_t, kind, out, workspace):
    """stationary_mll_sums, and se_mll_sums with kind "se", under the `name` their messages carry."""
    x, ldx, h, ldh, alpha_t, lda = _sums_operands(x, h, alpha_t, name)
    n, d = x.shape
    p = alpha_t.shape[0]
    code = _kind(kind, name)
    rc, plan = gp_mll_plan_status(n, d, p)
    _lib.check(rc, name)
    workspace, out = _sums_buffers(workspace, out, plan, 3, x.device, name)
    _lib.check(_lib.load().pg_gp_stat_mll_sums(code, x.data_ptr(), ldx, n, d, float(std), float(lengthscale), h.data_ptr(), ldh,
                                               alpha_t.data_ptr(), lda, p, workspace.data_ptr(), workspace.numel(), out.data_ptr(), _stream()),
               "pg_gp_stat_mll_sums")
    return out


def ard_mll_sums(x, std, lengthscale, h, alpha_t, *, kind="se", out=None, workspace=None, inv_lengthscale=None):
    """The gradients of the log marginal likelihood with respect to std, noise_var and EVERY per-dimension lengthscale, for the
    rows of x (n, d), h (n, n) = K^-1 (only its lower triangle is read) and alpha_t (p, n): the 1-D tensor of d + 2 floats
        (sum_ij G_ij K_f,ij / std,  tr G / 2,  S_0 / (2 l_0), ..., S_{d-1} / (2 l_{d-1})),
        S_c = sum_ij G_ij std^2 omega(r_ij) ((x_ic - x_jc) / l_c)^2,   G = alpha alpha^T - p h,
    on the GPU, into `out` if given. lengthscale: a 1-D fp32 tensor of d entries on the GPU (inv_lengthscale: its reciprocal, if
    the caller keeps one). One workgroup per 64 x 64 tile on or below the diagonal; the per-dimension terms are exact
    differences on the VALU, the rows of x staged in chunks of 64 columns; nothing of size (n, n) is written. `workspace`
    (ops.gp_ard_plan's workspace_floats, made if not given) takes one fp32 partial row of d + 2 floats per tile, which a second
    launch adds in double in a fixed order. d <= 256 (ValueError above). No atomics: bit-identical from run to run. Two
    launches, capturable."""
    name = "ard_mll_sums"
    x, ldx, h, ldh, alpha_t, lda = _sums_operands(x, h, alpha_t, name)
    n, d = x.shape
    p = alpha_t.shape[0]
    code = _kind(kind, name)
    if inv_lengthscale is None and not torch.is_tensor(lengthscale):
        raise ValueError(f"{name}: lengthscale must be a 1-D tensor of {d} entries (stationary_mll_sums takes a shared float)")
    _, inv = _lengthscale(lengthscale, inv_lengthscale, d, name)
    rc, plan = gp_ard_plan_status(n, d, p)
    _lib.check(rc, name)
    workspace, out = _sums_buffers(workspace, out, plan, d + 2, x.device, name)
    _lib.check(_lib.load().pg_gp_ard_mll_sums(code, x.data_ptr(), ldx, n, d, float(std), inv.data_ptr(), h.data_ptr(), ldh, alpha_t.data_ptr(),
                                              lda, p, workspace.data_ptr(), workspace.numel(), out.data_ptr(), _stream()),
               "pg_gp_ard_mll_sums")
    return out
