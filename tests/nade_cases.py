"""The shapes and inputs of the NADE tests (tests/test_nade_cpu.py checks the conditions they rest on, tests/test_gpu_nade.py
runs them).

Geometry constants as ops.nade_plan reports them (test_nade_cpu.py holds the two together): the chunk length over D, the samples
of a forward workgroup, the samples of a backward tile and the cap of the partial rows.

EXACT cases: x in {0, 1}, in_w and in_b on the grid 2^-10 Z with |w| < 4, D <= 784. Every partial sum of the recurrence is a
multiple of 2^-10 below 2^12 and fits fp32's 24 bits, so the fp32 recurrence equals the float64 one exactly and the ReLU masks
cannot differ. h_w, h_b and the incoming gradient are Gaussian.

GENERIC cases: Gaussian weights and real x of either sign, N D H <= 10^4, with the first seed for which min |a_i[n, h]| in
float64 is at least 1e-4 (a ReLU whose argument sits on zero would make the float64 gradient an arbitrary yardstick)."""

import torch

import _nade_ref as nref

CHUNK, TILE, BWD_TILE, MAX_ROWS = 32, 64, 16, 16
MAX_H = 8192
GENERIC_MARGIN = 1e-4

D_LIST = (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
H_LIST = (1, 63, 64, 65, 500)
# 1, 2, the forward workgroup's samples +- 1, and MAX_ROWS backward tiles plus a ragged one: the first partial row loops twice
N_LIST = (1, 2, TILE - 1, TILE + 1, BWD_TILE * MAX_ROWS + 5)
RECIPE = (784, 500, 70)
FULL_TILE = (CHUNK + 1, 65, TILE)  # no ragged tile, forward or backward
EXACT_SHAPES = [(d, h, n) for d in D_LIST for h in H_LIST for n in N_LIST] + [FULL_TILE, RECIPE]
GENERIC_SHAPES = [(33, 65, 4), (67, 9, 16), (1, 500, 17), (40, 1, 65), (5, 20, 70), (12, 20, 5)]


def shape_id(shape):
    return "d{}-h{}-n{}".format(*shape)


def _gen(shape, salt):
    d, h, n = shape
    return torch.Generator().manual_seed(((d * 1009 + h) * 1013 + n) * 31 + salt)


def exact_inputs(shape):
    """{x, _in_W, _in_b, _h_W, _h_b, g} of an exact case, float32 on the CPU."""
    d, h, n = shape
    g = _gen(shape, 0)
    grid = lambda *size: torch.randint(-4095, 4096, size, generator=g).float() / 1024  # noqa: E731
    return {"x": torch.bernoulli(torch.full((n, d), 0.4), generator=g), "_in_W": grid(h, d), "_in_b": grid(h),
            "_h_W": torch.randn(d, h, generator=g) / h ** 0.5, "_h_b": torch.randn(d, generator=g) * 0.3,
            "g": torch.randn(n, d, generator=g)}


def _generic(shape, salt):
    d, h, n = shape
    g = _gen(shape, 1000 + salt)
    return {"x": torch.randn(n, d, generator=g), "_in_W": torch.randn(h, d, generator=g) / d ** 0.5,
            "_in_b": torch.randn(h, generator=g) * 0.3, "_h_W": torch.randn(d, h, generator=g) / h ** 0.5,
            "_h_b": torch.randn(d, generator=g) * 0.3, "g": torch.randn(n, d, generator=g)}


def generic_inputs(shape, max_tries=50):
    """The inputs of the first seed whose smallest |a_i[n, h]| in float64 is at least GENERIC_MARGIN, and that margin."""
    assert shape[0] * shape[1] * shape[2] <= 10 ** 4
    for salt in range(max_tries):
        t = _generic(shape, salt)
        margin = float(nref.preact(t["x"], t["_in_W"], t["_in_b"]).abs().min())
        if margin >= GENERIC_MARGIN:
            return t, margin
    raise RuntimeError(f"no seed within {max_tries} tries for {shape}")


def params(t):
    return [t[k] for k in nref.KEYS]
