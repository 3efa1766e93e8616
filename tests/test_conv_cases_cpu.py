"""CPU: the case table of tests/_conv_cases.py (the forward / data-gradient convolutions tests/test_gpu_conv_families.py runs).

  * every bf16x3 case lands on the kernel instantiation its entry names (pg_conv_b3_route), for every input kind, with the
    misalignment flag where the entry has the letter; the fp32-MFMA and tap cases get their format from pg_conv_mfma_supported;
  * every distinct (kernel, MT, CG, MS, GT, gelu, two_tiles) among the bench workloads' routes (tests/golden/conv_b3_routes.json) is
    reached by a case;
  * the hand-written float64 reference agrees with float64 F.conv2d (autograd for the data gradients) and an epilogue written with
    torch's own functions, to 1e-12;
  * the exactness bound: in the four exact kinds sum |w| |in_act(x)| + |bias| + |res| + |res2| stays below 2^24 units at every
    output, and every input is a multiple of the unit — what lets the GPU test demand the reference bit for bit;
  * the inputs discriminate: the emulated six-product sum equals the reference exactly, leaving out any product the kind is said to
    exercise changes it, and the three products the kernels drop are identically zero;
  * the pieces are populated: three non-zero x pieces in x3, three non-zero w pieces in w3, two each in x2w2."""

import json
import os

import numpy as np
import pytest
import torch

import _conv_b3_routes as R
import _conv_cases as V
import _util

B3 = V.B3_CASES


@pytest.mark.parametrize("case", B3, ids=lambda c: c.name)
def test_case_lands_where_its_entry_says(lib, case):
    c = case
    assert V.fmt_of(lib, c) == V.FMT_B3, c.name
    keys = set()
    for kind in V.KINDS:
        r = V.route(lib, c, kind)
        assert not V.route_problems(c, r, kind), (c.name, kind, V.route_problems(c, r, kind), r)
        assert bool(V.flags_of(c, kind) & R.IN_MISALIGNED) == ("in" in c.mis)
        keys.add(V.key_of(r)[:5] + V.key_of(r)[6:])  # the GELU instantiation aside, every kind runs the same kernel
        if c.form == "plain":  # the fused single residual of the plain form stays on the same instantiation
            assert V.key_of(V.route(lib, c, kind, fused_res=True)) == V.key_of(r), (c.name, kind)
    assert len(keys) == 1, (c.name, keys)
    if "in" in c.mis:  # the flag is what moves it: the aligned twin takes the 1x1 kernel
        pr = V.problem(c, "int")
        rc, r = R.route(lib, dict(pr, flags=pr["flags"] & ~R.IN_MISALIGNED))
        assert rc == 0 and R.named(r)["kernel"] == V.PW, c.name


@pytest.mark.parametrize("case", [c for c in V.CASES if c.backend != "b3"], ids=lambda c: c.name)
def test_other_backends_get_their_format(lib, case):
    assert V.fmt_of(lib, case) == V.FMT_OF_BACKEND[case.backend], case.name


def test_table_covers_what_it_is_for(lib):
    rts = {(c.name, k): V.route(lib, c, k) for c in B3 for k in V.KINDS}
    keys = {V.key_of(r) for r in rts.values()}
    names = {k[0] for k in keys}
    assert names == {"staged", "1x1", "pipelined", "overlapped"}
    # staged: one to four output tiles, narrow and wide, both multi-stream forms, the gate, one to four pixel groups per wave
    staged = {k for k in keys if k[0] == "staged"}
    assert {k[1] for k in staged} == {1, 2, 3, 4} and {k[7] for k in staged} == {1, 2, 3, 4}
    assert {(k[2], k[3], k[4]) for k in staged} == {(1, 0, 0), (1, 1, 0), (2, 0, 0), (2, 1, 0), (2, 0, 1)}
    assert {(k[1], k[3]) for k in keys if k[0] == "1x1"} == {(1, 0), (2, 0), (4, 0), (4, 1)}
    assert {k[7] for k in keys if k[0] == "pipelined"} == {1, 2}
    assert any(k[5] for k in staged) and any(k[5] for k in keys if k[0] == "1x1")  # both GELU translation units
    # every epilogue form on the staged and the 1x1 kernel, the multi-stream ones on the pipelined and the overlapped too
    forms = {(R.KERNELS[rts[c.name, "int"]["kernel"]], c.form) for c in B3}
    assert {("staged", f) for f in ("plain", "two_residuals", "same_residual_twice", "res_dact", "res_strided", "gate")} <= forms
    assert {("1x1", f) for f in ("plain", "two_residuals", "same_residual_twice", "res_dact", "dual")} <= forms
    assert {("pipelined", "two_residuals"), ("pipelined", "res_dact"), ("overlapped", "two_residuals")} <= forms
    # tiles: several row tiles per image with a ragged last one, an odd batch on the overlapped kernel's pairs, a partial chunk
    assert any(r["tiles_per_img"] > 1 and V.BY_NAME[n].oh % r["TR"] for (n, _), r in rts.items())
    assert any(c.n % 2 for c in B3 if rts[c.name, "int"]["kernel"] == V.OV)
    assert any(c.m % 64 for c in B3 if rts[c.name, "int"]["kernel"] in (V.ST, V.PL))
    assert {"fwd", "dgrad"} == {c.orient for c in V.CASES} and {2, 3} == {c.n for c in V.CASES}
    assert set(V.PACK2_CASES) <= set(V.BY_NAME)


# instantiations of the bench table no case reaches: (kernel, MT, CG, MS, GT, gelu, two_tiles) -> why
NOT_REACHED = {}


def test_every_instantiation_of_the_bench_workloads_has_a_case(lib):
    with open(os.path.join(_util.GOLDEN_DIR, "conv_b3_routes.json")) as f:
        gold = json.load(f)
    idx = [R.FIELDS.index(k) for k in V.KEY_FIELDS]
    bench = {tuple(r[i] for i in idx) for _, _, r in R.unpack_table(gold["table"])}
    ours = set()
    for c in B3:
        for kind in V.KINDS:
            r = V.route(lib, c, kind)
            ours.add(tuple(r[k] for k in V.KEY_FIELDS))
    missing = {k for k in bench if k not in ours and k not in NOT_REACHED}
    assert not missing, f"bench instantiations (kernel, MT, CG, MS, GT, gelu, two_tiles) without a case: {sorted(missing)}"
    assert not [k for k in NOT_REACHED if k in ours], "an exception that is reached after all"


@pytest.mark.parametrize("case", V.CASES, ids=lambda c: c.name)
def test_reference_agrees_with_torch_and_the_exact_kinds_are_exact(case):
    c = case
    for kind in V.KINDS:
        d = V.inputs(c.name, kind)
        a = V.acts_of(c, kind)
        for fused in ((False, True) if c.form == "plain" else (False,)):
            ref, want = V.reference(c.name, kind, fused), V.torch_reference(c, kind, d, fused)
            assert set(ref) == set(want)
            for k in ref:
                scale = float(want[k].abs().max().clamp_min(1.0))
                assert float((ref[k] - want[k]).abs().max()) <= 1e-12 * scale, (c.name, kind, k)
        if kind == "random":
            continue
        unit = V.UNIT[kind]
        assert a["in_act"] in (0, 1) and a["out_act"] in (0, 1) and (a["dact"] in (0, 1) or c.form == "dual")
        operands = [d["x"], d["w"], d["res"], d["res2"], d["gate_res"], d["dact_src"], d["r"]] + ([] if d["bias"] is None else [d["bias"]])
        for t in operands:  # every input a multiple of the unit
            q = t.double() / unit
            assert bool((q == q.round()).all()), (c.name, kind)
        per_row = (V.wsel_of(c, d["w"]) != 0).reshape(c.m, -1).sum(dim=1)
        assert int(per_row.max()) <= V.NNZ[kind] and (kind == "int" or int(per_row.min()) >= 1), (c.name, kind, int(per_row.max()))
        if c.form == "dual":
            y = d["dact_src"] - d["r"]
            assert bool((d["dact_src"] > 0).all()) and float(y.min()) >= -2 and float(d["r"].min()) >= -2
        for fused in ((False, True) if c.form == "plain" else (False,)):
            bound = V.reference_of(c, kind, d, fused, absolute=True)["out"]
            assert float(bound.max()) / unit + 3 < 2 ** 24, (c.name, kind, float(bound.max()) / unit)
            for k, v in V.reference(c.name, kind, fused).items():
                if k != "gate_out":  # (a function of the exact `out`, not exact itself)
                    assert bool((v.float().double() == v).all()), (c.name, kind, k)
                    assert bool(((v / unit) == (v / unit).round()).all()), (c.name, kind, k)


DISCRIMINATION_CASES = ("staged-3x3-64to64", "pw-64to64-two-residuals", "pipelined-2x2-64to64-dgrad-res-dact",
                        "overlapped-2x3-256to64-12x32", "gate-1x3-32to128-12x12", "dgrad-2x3-320to16-staged-narrow")


@pytest.mark.parametrize("kind", V.EXACT_KINDS)
@pytest.mark.parametrize("name", DISCRIMINATION_CASES)
def test_inputs_discriminate_between_the_six_products(name, kind):
    c, d = V.BY_NAME[name], V.inputs(name, kind)
    ref = V.reference(name, kind)["out"]
    assert torch.equal(V.six_products(c, kind, d)["out"], ref), (name, kind)
    for p in V.EXERCISES[kind]:
        without = V.six_products(c, kind, d, without=(p,))["out"]
        changed = float((without != ref).double().mean())
        # (a ReLU output activation clips about half of the outputs to zero with or without the product, a ReLU derivative zeroes
        # four in seven: a quarter to a fifth of the outputs is what can change at the least)
        assert changed > 0.15, f"{name} ({kind}): leaving out {p} changes only {changed:.0%} of the outputs"
        assert float((without - ref).abs().max()) >= V.UNIT[kind]
    for p in V.DROPPED:
        assert not bool(V.six_products(c, kind, d, only=(p,)).any()), (name, kind, p)
    for p in set(V.PRODUCTS) - set(V.EXERCISES[kind]):  # (what the kind does not exercise is absent, not merely small)
        assert not bool(V.six_products(c, kind, d, only=(p,)).any()), (name, kind, p)


@pytest.mark.parametrize("case", V.CASES, ids=lambda c: c.name)
def test_pieces_are_populated(case):
    c = case

    def filled(pieces, where):
        return [float(((p != 0) & where).sum() / where.sum()) for p in pieces]

    x = V.inputs(c.name, "x3")["x"].numpy()
    assert min(filled(V.split8t(x), x != 0)) >= 0.9 and float((x != 0).mean()) == 1.0, c.name
    w = V.wsel_of(c, V.inputs(c.name, "w3")["w"]).numpy()
    assert min(filled(V.split8(w), w != 0)) >= 0.9, c.name
    xm, wm = V.inputs(c.name, "x2w2")["x"].numpy(), V.wsel_of(c, V.inputs(c.name, "x2w2")["w"]).numpy()
    fx, fw = filled(V.split8t(xm), xm != 0), filled(V.split8(wm), wm != 0)
    assert min(fx[:2]) >= 0.9 and fx[2] == 0.0 and min(fw[:2]) >= 0.9 and fw[2] == 0.0, c.name
    # the splits are exact: the pieces sum to the value
    for split, v in ((V.split8t, x), (V.split8, w), (V.split8t, xm), (V.split8, wm)):
        h, m, lo = split(v)
        assert np.array_equal(h.astype(np.float64) + m + lo, v.astype(np.float64)), c.name
