"""CPU: `pg_attn_route`, the host-only export of the one function (csrc/attention.hip: attn_route) from which every causal
attention launch takes its kernel family, template instantiation, grid and tile sizes.

Checks that every case of tests/_attn_cases.py lands on the family and has the feature its entry claims (so the GPU tests of
tests/test_gpu_attention_families.py run what they say they run), the invariants of the geometry the route reports over a sweep
of shapes, the band edges of the d_k = d_v = 4 family (found by scanning L, not written down here), and what misaligned planes
and strides do to a k4 shape."""

import pytest

import _attn_cases as A

FWD, DQ, DKV, BWD = A.FWD, A.DQ, A.DKV, A.BWD
LDS_MAX = 160 * 1024
LDS_VALU_MAX = 64 * 1024


@pytest.fixture(scope="module")
def ops(lib):
    from pytorch_generative_amd import ops

    assert lib.pg_attn_fused_bwd(-1) == 1, "the fused backward is on by default"
    return ops


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.name)
def test_case_lands_where_its_entry_says(ops, lib, case):
    rts = A.routes(case)
    assert not A.route_problems(case, rts), (case.name, A.route_problems(case, rts), rts)
    # the switch off: the fused request is declined, nothing else moves; the route reads the switch and leaves it alone
    assert lib.pg_attn_fused_bwd(0) == 1
    try:
        off = A.routes(case)
        assert lib.pg_attn_fused_bwd(-1) == 0
    finally:
        lib.pg_attn_fused_bwd(1)
    assert not A.route_problems(case, off, fused_on=False), (case.name, A.route_problems(case, off, fused_on=False))
    assert all(r["fused_on"] == 0 for r in off) and all(r["fused_on"] == 1 for r in rts)
    strip = lambda r: {k: v for k, v in r.items() if k != "fused_on"}  # noqa: E731
    assert [strip(r) for r in off[:3]] == [strip(r) for r in rts[:3]]
    assert A.routes(case) == rts


def test_case_table_covers_what_it_is_for():
    feats = {f for c in A.CASES for f in c.features}
    assert feats == set(A.FEATURES), set(A.FEATURES) - feats
    valu = [c for c in A.CASES if A.family_of(c) == "valu"]
    assert {c.strict for c in valu} == {False, True} and all(c.n <= 2 for c in valu)
    k4 = {(c.dk, c.dv) for c in A.CASES if A.family_of(c) == "k4" and 64 <= c.h * c.w <= 400}
    assert k4 == {(dk, dv) for dk in (4, 16, 32, 64) for dv in (16, 32, 64)}
    assert any(c.merged for c in A.CASES if A.family_of(c) == "m44") and any(c.merged for c in valu)


SWEEP_DIMS = [(1, 1), (2, 2), (3, 7), (4, 4), (4, 5), (4, 16), (4, 17), (4, 32), (4, 64), (8, 8), (8, 16), (16, 4), (16, 16),
              (16, 32), (16, 64), (32, 16), (32, 32), (32, 64), (64, 16), (64, 32), (64, 64)]
SWEEP_L = [1, 15, 16, 17, 63, 64, 65, 128, 144, 169, 448, 449, 512, 513, 768, 784, 1024, 1025, 1089, 2048, 2049, 2116, 3481, 4097]


def test_route_geometry_invariants(ops):
    seen = set()
    for dk, dv in SWEEP_DIMS:
        for L in SWEEP_L:
            for n, heads in ((1, 1), (3, 2), (768, 2)):
                for which in (FWD, DQ, DKV, BWD):
                    r = ops.attention_route(which, n, heads, L, dk, dv)
                    what = (which, n, heads, L, dk, dv, r)
                    native = which == BWD or ops.attention_dims_native(dk, dv, L)
                    assert (r["status"], r["family"] == "none") == ((0, False) if native else (-2, True)), what
                    if not native:
                        continue
                    seen.add((r["family"], which))
                    nb = -(-L // 64)
                    if r["family"] == "declined":
                        assert which == BWD and r["grid_x"] == 0, what
                        continue
                    assert 0 <= r["lds"] <= LDS_MAX and r["block"] % 64 == 0 and 64 <= r["block"] <= 512, what
                    assert r["grid_x"] >= 1 and r["grid_y"] >= 1 and r["grid_z"] >= 1, what
                    if r["family"] == "valu":
                        assert which != BWD and r["lds"] <= LDS_VALU_MAX, what
                        assert (r["grid_y"], r["grid_z"]) == (heads, n), what
                        assert r["t0"] >= dk and r["t1"] >= dv and (r["t0"], r["t1"]) in ((4, 4), (4, 16), (4, 32), (16, 4), (16, 16))
                        assert r["kt"] % 64 == 0 and 64 <= r["kt"] <= 64 * nb, what
                        assert r["tiles"] == -(-L // r["kt"]), what
                        assert 1 <= r["blocks_per_wg"] <= 16 and r["blocks_per_wg"] == min(nb, 16), what
                        assert r["grid_x"] == -(-nb // r["blocks_per_wg"]), what          # every block has a workgroup
                        assert r["waves"] == -(-r["blocks_per_wg"] // 2) and r["block"] == 64 * r["waves"], what
                        row = r["t0"] + r["t1"] + (4 if which == DKV else 0)              # floats per staged row
                        assert r["lds"] == 4 * r["kt"] * row, what
                    elif r["family"] == "m44":
                        assert (dk, dv) == (4, 4) and (r["grid_x"], r["grid_y"], r["grid_z"]) == (1, heads, n), what
                        assert r["lp"] == 64 * nb + 16 and r["vec"] == (1 if L % 4 == 0 else 0), what
                        assert 1 <= r["waves"] <= min(8, nb) and r["block"] == 64 * r["waves"], what
                        assert nb <= 16 * r["waves"], what                                 # a wave's list holds 16 blocks
                    else:
                        assert r["family"] == "k4" and L % 16 == 0 and dk in (4, 16, 32, 64) and dv in (16, 32, 64), what
                        assert (r["t0"], r["t1"]) == A._k4_inst(dk, dv) and r["qb"] in (1, 2, 4), what
                        assert r["block"] == 64 and r["lds"] == 0 and r["grid_x"] % 64 == 0, what
                        pairs = -(-(-(-L // (16 * r["qb"]))) // 2)
                        assert r["grid_x"] == 64 * -(-n * heads // 64) * pairs, what      # every block pair of every unit
                        if which == BWD:
                            assert dk == 4 and dv <= 32 and r["qb"] == 2, what
    assert {("valu", FWD), ("valu", DKV), ("m44", BWD), ("k4", BWD), ("k4", DQ), ("m44", FWD), ("declined", BWD)} <= seen


def test_uninstantiated_shapes_return_the_launch_status(ops, lib):
    from test_host_cpu import _fake_ptr

    for dk, dv, L in [(24, 40, 45), (32, 32, 100), (4, 64, 49), (16, 32, 17), (5, 17, 16), (4, 33, 64), (17, 4, 64)]:
        for which in (FWD, DQ, DKV):
            r = ops.attention_route(which, 1, 1, L, dk, dv)
            assert (r["status"], r["family"]) == (-2, "none"), (which, dk, dv, L, r)
            assert ops.attention_dims_native(dk, dv, L) is False
        assert ops.attention_route(BWD, 1, 1, L, dk, dv)["family"] == "declined"
    # ... the same status the launch itself gives: it asks the route before any device call, so nothing is launched and the
    # pointers are never read
    keep, p = _fake_ptr()
    assert lib.pg_causal_attn_fwd(p, p, p, p, p, 1, 1, 45, 24, 40, 24 * 45, 64 * 45, 64 * 45, 40 * 45, 1, None) == -2
    assert b"not instantiated" in lib.pg_last_error()
    assert lib.pg_causal_attn_bwd(*[p] * 10, 1, 1, 45, 24, 40, *[64 * 45] * 8, 1, None) == -2
    del keep
    out = __import__("pytorch_generative_amd")._lib.int_array([7] * 17)
    assert lib.pg_attn_route(0, 1, 1, 64, 4, 4, 0, out, 16) == -1 and list(out) == [7] * 17      # short array
    assert lib.pg_attn_route(0, 1, 1, 64, 4, 4, 0, None, 17) == -1
    assert lib.pg_attn_route(4, 1, 1, 64, 4, 4, 0, out, 17) == -1
    assert lib.pg_attn_route(0, 1, 1, 0, 4, 4, 0, out, 17) == -1
    assert lib.pg_attn_route(0, 1, 1, 64, 65, 4, 0, out, 17) == -2
    assert list(out) == [7] * 17


def test_everything_native_has_a_route(ops):
    """ops.attention_dims_native (what the Python host sends to the kernels unpadded) and the route agree, with the
    layouts ops.causal_attention and ops.causal_attention_qkv produce."""
    dims = (1, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33, 48, 63, 64)
    for dk in dims:
        for dv in dims:
            for L in (1, 16, 45, 48, 49, 64, 100, 144):
                for merged in (False, True):
                    flags = ops.attention_layout_flags(1, dk, dv, L, merged)
                    ok = all(ops.attention_route(w, 2, 1, L, dk, dv, flags)["status"] == 0 for w in (FWD, DQ, DKV))
                    assert ok == ops.attention_dims_native(dk, dv, L), (dk, dv, L, merged)


def _edges(ops, which):
    """[(L, family at L - 1, family at L)] wherever the family of `which` changes for d_k = d_v = 4. A route of this family
    makes the block plan of its L (a search of milliseconds), so the scan visits both sides of every 64-row block boundary
    and two lengths inside every block instead of every L; that the budget moves with whole blocks only is asserted by the
    caller (lp, the plane arithmetic) rather than assumed."""
    visit = sorted({L for b in range(0, 4224, 64) for L in (b, b + 1, b + 17, b + 40) if 1 <= L < 4200})
    fam = {L: ops.attention_route(which, 1, 2, L, 4, 4)["family"] for L in visit}
    edges = [(b, fam[a], fam[b]) for a, b in zip(visit, visit[1:]) if fam[a] != fam[b]]
    assert all(b % 64 == 1 for b, _, _ in edges), edges  # every change found lies between L = 64 k and 64 k + 1
    return edges


def test_d4_band_edges_are_in_the_case_table(ops):
    d4 = {c.h * c.w for c in A.CASES if c.dk == 4 and c.dv == 4}
    lasts = {}
    for which, gone in ((FWD, "valu"), (DQ, "valu"), (DKV, "valu"), (BWD, "declined")):
        edges = _edges(ops, which)
        assert len(edges) == 1 and edges[0][1:] == ("m44", gone), (which, edges)  # one band per kernel, never back
        first_off = edges[0][0]
        assert first_off - 1 in d4 and first_off in d4, (A.KERNELS[which], first_off - 1, first_off, sorted(d4))
        assert (first_off - 1) % 64 == 0  # the planes grow with 64-row blocks
        lasts[which] = first_off - 1
        # the budget itself: the reported LDS fits before the edge and the next block's planes would not
        r = ops.attention_route(which, 1, 2, first_off - 1, 4, 4)
        planes = (r["lds"] - (8192 if which == BWD else 16)) // (4 * r["lp"])
        assert r["lds"] <= LDS_MAX < 4 * planes * (r["lp"] + 64) + (8192 if which == BWD else 16), (which, r)
    assert lasts[BWD] < lasts[DQ] < lasts[DKV] < lasts[FWD]  # hence the mixed bands the d4-* cases are named for
    # every band between two edges has a case strictly inside it
    for lo, hi in ((lasts[BWD], lasts[DQ]), (lasts[DQ], lasts[DKV]), (lasts[DKV], lasts[FWD]), (lasts[FWD], 4200)):
        assert any(lo + 1 < L < hi for L in d4), (lo, hi)


def test_misalignment_moves_a_k4_shape(ops):
    """pg_attn_k4_route's conditions on pointers and strides: a shape it would take goes to the VALU family when that one
    instantiates the head dims, to PG_ESHAPE when not; flags the kernel in question never reads change nothing."""
    o = __import__("pytorch_generative_amd").ops.attention
    every = [o.ATTN_R_QKV_MISALIGNED, o.ATTN_R_O_MISALIGNED, o.ATTN_R_GRADIN_MISALIGNED, o.ATTN_R_DQ_MISALIGNED,
             o.ATTN_R_DKV_MISALIGNED, o.ATTN_R_QKV_STRIDE, o.ATTN_R_O_STRIDE, o.ATTN_R_DO_STRIDE, o.ATTN_R_DQ_STRIDE,
             o.ATTN_R_DKV_STRIDE]
    fwd_reads = {o.ATTN_R_QKV_MISALIGNED, o.ATTN_R_QKV_STRIDE, o.ATTN_R_O_STRIDE}
    bwd_reads = fwd_reads | {o.ATTN_R_GRADIN_MISALIGNED, o.ATTN_R_DO_STRIDE, o.ATTN_R_DQ_STRIDE, o.ATTN_R_DKV_STRIDE}
    fused_reads = bwd_reads | {o.ATTN_R_DQ_MISALIGNED}
    for dk, dv, fallback in [(4, 32, "valu"), (4, 16, "valu"), (16, 16, "valu"), (32, 32, "none"), (4, 64, "none"),
                             (16, 32, "none")]:
        for which, reads in ((FWD, fwd_reads), (DQ, bwd_reads), (DKV, bwd_reads), (BWD, fused_reads)):
            clean = ops.attention_route(which, 2, 2, 144, dk, dv)
            if which == BWD and not (dk == 4 and dv <= 32):
                assert clean["family"] == "declined"
                continue
            assert clean["family"] == "k4"
            for flag in every:
                r = ops.attention_route(which, 2, 2, 144, dk, dv, flag)
                if flag not in reads:
                    assert r == clean, (which, dk, dv, flag)
                elif which == BWD:
                    assert (r["family"], r["status"]) == ("declined", 0), (dk, dv, flag, r)
                else:
                    assert (r["family"], r["status"]) == (fallback, 0 if fallback == "valu" else -2), (which, dk, dv, flag, r)
    # d_k = d_v = 4: misaligned outputs keep the family and drop the float4 stores
    for which, flag in ((FWD, o.ATTN_R_O_MISALIGNED), (FWD, o.ATTN_R_O_STRIDE), (DQ, o.ATTN_R_DQ_MISALIGNED),
                        (DQ, o.ATTN_R_DQ_STRIDE), (DKV, o.ATTN_R_DKV_STRIDE), (BWD, o.ATTN_R_DKV_MISALIGNED)):
        clean, r = ops.attention_route(which, 2, 2, 784, 4, 4), ops.attention_route(which, 2, 2, 784, 4, 4, flag)
        assert clean["vec"] == 1 and r == dict(clean, vec=0), (which, flag)
    assert ops.attention_route(FWD, 2, 2, 784, 4, 4, o.ATTN_R_QKV_MISALIGNED)["vec"] == 1
