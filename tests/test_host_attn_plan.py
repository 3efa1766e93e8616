"""CPU: `pg_attn_block_plan`, the host-only export of the block plan that `pg_attn_mfma_launch` hands to the
d_k = d_v = 4 matrix-core attention kernels (csrc/attention_mfma.hip) — which blocks exist, which wave walks which.

Query-owner kernels (forward, dQ): with G = ceil(L / 16) groups and F = G mod 4, block 0 is the first F groups (all
four when F = 0) and every later block holds four, so no block streams keys for queries that do not exist; the cost
of a block is the number of 16-query group evaluations the kernel issues for it, and the assignment to waves must be
at least as good as longest-processing-time-first on those costs — for the lengths here it is the optimum.
Key-owner kernels (dK/dV, fused backward): the plan is the rule they have always had, restated literally below."""

import pytest

FWD, DQ, DKV, BWD = 0, 1, 2, 3
LENGTHS = [16, 48, 64, 80, 100, 117, 224, 784, 1024, 1040]


def _plan(lib, which, L, waves):
    """[(block, q0, ngrp, wave, cost)] in the order of the export: wave by wave, each wave's list in walking order."""
    from pytorch_generative_amd import _lib

    nb = -(-L // 64)
    out = [_lib.int_array([-1] * nb) for _ in range(5)]
    n = lib.pg_attn_block_plan(which, L, waves, *out)
    assert n == nb, (which, L, waves, n)
    return list(zip(*(list(a) for a in out)))


def _loads(plan):
    loads = {}
    for _, _, _, wave, cost in plan:
        loads[wave] = loads.get(wave, 0) + cost
    return loads


def _query_blocks(L):
    """(q0, ngrp, cost) of the forward / dQ blocks, written out from the kernels' walk: block 0 runs one tile step
    per group it owns, step u evaluating groups u..3; a later block runs q0 / 16 tiles below it with all four groups
    and its four diagonal steps with 4, 3, 2, 1."""
    groups = -(-L // 16)
    first = groups % 4 or 4
    blocks = [(0, first, sum(4 - u for u in range(first)))]
    for q0 in range(16 * first, 16 * groups, 64):
        blocks.append((q0, 4, 4 * (q0 // 16) + 10))
    return blocks


def _greedy_max(costs, waves):
    load = [0] * waves
    for c in sorted(costs, reverse=True):
        load[load.index(min(load))] += c
    return max(load)


def _optimal_max(costs, waves, bound):
    """Smallest possible maximum wave load: every assignment, as the set of sorted load vectors after each block
    (heaviest first), dropping only vectors already above `bound`, a value known to be attainable."""
    states = {(0,) * waves}
    for c in sorted(costs, reverse=True):
        nxt = set()
        for s in states:
            for w in range(waves):
                if w and s[w] == s[w - 1]:
                    continue
                t = list(s)
                t[w] += c
                if t[w] <= bound:
                    nxt.add(tuple(sorted(t, reverse=True)))
        states = nxt
    return min(s[0] for s in states)


@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("which", [FWD, DQ], ids=["fwd", "dq"])
@pytest.mark.parametrize("L", LENGTHS)
def test_query_owner_plan(lib, L, which, waves):
    plan = _plan(lib, which, L, waves)
    groups = -(-L // 16)
    want = _query_blocks(L)
    assert len(want) == -(-L // 64)
    # the blocks tile [0, 16 G) exactly once; every block but the first has four groups; costs are the kernel's
    by_block = sorted(plan)
    assert [b for b, *_ in by_block] == list(range(len(want)))
    assert [(q0, ngrp, cost) for _, q0, ngrp, _, cost in by_block] == want
    covered = [g for _, q0, ngrp, _, _ in by_block for g in range(q0 // 16, q0 // 16 + ngrp)]
    assert covered == list(range(groups))
    assert all(ngrp == 4 for _, _, ngrp, _, _ in by_block[1:]) and all(q0 % 16 == 0 for _, q0, *_ in by_block)
    # every block on exactly one wave (one entry each, above), at most 16 per wave, each list in decreasing cost
    used = min(waves, len(want))
    for w in range(used):
        mine = [cost for _, _, _, wave, cost in plan if wave == w]
        assert len(mine) <= 16 and mine == sorted(mine, reverse=True), (w, mine)
    assert all(0 <= wave < used for _, _, _, wave, _ in plan)
    assert [wave for _, _, _, wave, _ in plan] == sorted(wave for _, _, _, wave, _ in plan)
    # balance: never worse than greedy on the same costs, and for these lengths the optimum
    costs = [c for _, _, c in want]
    got, greedy = max(_loads(plan).values()), _greedy_max(costs, used)
    assert got <= greedy
    assert got == _optimal_max(costs, used, greedy), (got, greedy)


def test_bench_length_plan_is_optimal(lib):
    """L = 784 on 4 waves: the short block is one step (4 units), the 12 full blocks cost 14, 30, .., 190 quarter
    steps. Brute force over every assignment of the full blocks (the heaviest pinned to wave 0: 4^11): with three
    blocks on every wave no maximum below 314 (78.5 steps) exists, with 4 + 4 + 2 + 2 blocks it is 312 — and that,
    the true optimum, is what the plan must reach; the short block rides on a lighter wave."""
    import numpy as np

    plan = _plan(lib, FWD, 784, 4)
    full = [14 + 16 * i for i in range(12)]
    assert sorted(c for *_, c in plan) == [4] + full
    idx = np.arange(4 ** 11, dtype=np.int32)
    load = np.zeros((4, idx.size), dtype=np.int32)
    count = np.zeros((4, idx.size), dtype=np.int8)
    load[0] += full[11]
    count[0] += 1
    for i in range(11):
        digit = (idx >> (2 * i)) & 3
        for w in range(4):
            on = digit == w
            load[w] += full[i] * on
            count[w] += on
    worst = load.max(axis=0)
    best = int(worst.min())
    assert int(worst[(count == 3).all(axis=0)].min()) == 314 and best == 312
    assert best == _optimal_max(full, 4, 330) == _optimal_max([4] + full, 4, 330)
    assert max(_loads(plan).values()) == best


def _key_owner_rule(L, waves):
    """The dK/dV / fused-backward rule as it has always been: 64-key blocks, block b has rank NB - 1 - b and cost
    4 * rank + 5; blocks in decreasing cost, each to the least loaded wave (lowest index on ties)."""
    nb = -(-L // 64)
    waves = min(waves, nb)
    load, lists = [0] * waves, [[] for _ in range(waves)]
    for rank in range(nb - 1, -1, -1):
        best = 0
        for w in range(1, waves):
            if load[w] < load[best] and len(lists[w]) < 16:
                best = w
        lists[best].append((nb - 1 - rank, 4 * rank + 5))
        load[best] += 4 * rank + 5
    return lists


# the rule's result at L = 784 on 4 and 8 waves, as the commit before the plan export launched it (its loop, compiled on
# its own and printed): guards the restatement above
KEY_OWNER_784 = {4: [[0, 7, 8], [1, 6, 9], [2, 5, 10], [3, 4, 11, 12]],
                 8: [[0], [1], [2], [3, 12], [4, 11], [5, 10], [6, 9], [7, 8]]}


@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("which", [DKV, BWD], ids=["dkv", "bwd"])
@pytest.mark.parametrize("L", LENGTHS)
def test_key_owner_plan_is_unchanged(lib, L, which, waves):
    for w8, lists in KEY_OWNER_784.items():
        assert [[b for b, _ in lst] for lst in _key_owner_rule(784, w8)] == lists
    plan = _plan(lib, which, L, waves)
    want = _key_owner_rule(L, waves)
    got = [[(b, c) for b, _, _, wave, c in plan if wave == w] for w in range(len(want))]
    assert got == want
    for b, q0, ngrp, _, _ in plan:
        assert q0 == 64 * b and ngrp == min(4, -(-(L - q0) // 16))


def test_plan_rejects_bad_arguments(lib):
    from pytorch_generative_amd import _lib

    out = [_lib.int_array([0] * 4) for _ in range(5)]
    assert lib.pg_attn_block_plan(4, 64, 4, *out) == -1
    assert lib.pg_attn_block_plan(FWD, 0, 4, *out) == -1
    assert lib.pg_attn_block_plan(FWD, 64, 9, *out) == -1
    assert lib.pg_attn_block_plan(FWD, 64, 4, None, *out[1:]) == -1
