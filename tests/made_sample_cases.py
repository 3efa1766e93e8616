"""The GPU parity cases of the one-launch MADE sampler, shared by tests/test_made_sampling_cpu.py (which shows that no draw of
any case sits closer to its threshold than the GPU's logit tolerance can move it, and that the shapes straddle every boundary
the plan has) and tests/test_gpu_made_sampling.py (which then demands exact samples).

A case is (n, D, H, seeds, givens): `givens` names the start canvases it is run with (made_sample_ref.GIVENS) and `seeds` the
seed of each — picked so that the margin condition of the CPU test holds; the float64 results are computed once per process."""

import functools

import made_sample_ref as mref

TILE = 4                 # the plan's samples per workgroup
H_BOUNDARIES = (64, 256, 1024, 4096)   # the last H of every (threads per workgroup, hidden units per thread) class
MAX_H = 8192
LOGIT_TOL = 1e-4         # _util.assert_close bound of the GPU logits: max |got - want| <= LOGIT_TOL * max |want|


def _case(n, d, h, seeds=(0, 0, 0)):
    return (n, d, h, tuple(seeds), mref.GIVENS)


CASES = [
    # the smallest shapes that can go wrong: one of everything, ragged, a full wave and one unit more, several tiles
    _case(1, 1, 1), _case(3, 13, 7), _case(5, 24, 64), _case(2, 24, 65), _case(37, 24, 300),
    # n at the tile (one below and one above are (3, 13, 7) and (5, 24, 64))
    _case(4, 13, 7),
    # D across the 64-step chunks in which the kernel keeps `order` in registers, odd and even
    _case(2, 65, 20), _case(3, 130, 40),
    # one H on each side of every plan boundary, and the last H of the domain
    _case(2, 24, 256), _case(2, 24, 257), _case(2, 24, 1024), _case(2, 24, 1025), _case(2, 24, 4096), _case(2, 24, 4097),
    _case(2, 24, 8192),
    # the recipe's network (1568 draws: seed 0 of the empty canvas has one at 3.8e-5 from its threshold, 6.1e-5 needed)
    _case(2, 784, 8000, seeds=(3, 0, 0)),
]


def case_id(case):
    return "n{}-d{}-h{}".format(*case[:3])


@functools.lru_cache(maxsize=None)
def net(d, h):
    return mref.masked_net(d, h, seed=1000 * d + h)


@functools.lru_cache(maxsize=None)
def build(n, d, h, givens, seed):
    """Inputs and float64 results of one run: dict(net=(w1, b1, w2, b2, order), canvas, uniforms, sample, logits)."""
    w = net(d, h)
    canvas, uniforms = mref.start_canvas(n, d, givens, seed)
    sample, logits = mref.chain(canvas, *w, uniforms)
    return {"net": w, "canvas": canvas, "uniforms": uniforms, "sample": sample, "logits": logits}


def runs(case):
    n, d, h, seeds, givens = case
    return [(n, d, h, g, s) for g, s in zip(givens, seeds)]
