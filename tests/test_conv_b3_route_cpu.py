"""CPU: the bf16x3 convolution's route (csrc/conv_b3.hip: b3_route, exported host-only as pg_conv_b3_route).

One function decides which kernel instantiation takes a problem and how it is laid out; the launch, pg_conv_dual_ok and
pg_conv_gate_fusable read its answer. tests/golden/conv_b3_routes.json holds what the launch did at the last commit that decided
inline (recorded through a capture hook, tests/golden/make_conv_b3_routes_golden.py): the route must reproduce it exactly."""

import ctypes
import json
import os

import pytest

import _conv_b3_routes as R
from test_host_cpu import _fake_ptr, _no_gpu, _reached_launch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_b3_routes.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def problems(lib):
    """Every problem of the two records: the bench workloads' table and the random sweep (bf16x3-routed problems only)."""
    table = [pr for _, pr in R.bench_problems(lib)]
    sweep = [pr for seed in range(4) for pr in R.random_problems(seed)]
    return table, sweep


def test_route_reproduces_the_recorded_table(lib, golden):
    assert golden["fields"] == R.FIELDS and golden["w9_plans"] == []
    rows, recorded = R.bench_problems(lib), R.unpack_table(golden["table"])
    assert [label for label, _ in rows] == [label for label, _, _ in recorded]
    kernels = set()
    for (label, pr), (_, geometry, want) in zip(rows, recorded):
        assert [pr[k] for k in R.GEOMETRY] == geometry, label
        rc, r = R.route(lib, pr)
        assert rc == 0, (label, rc, lib.pg_last_error())
        assert r == want, (label, {k: (a, b) for k, a, b in zip(R.FIELDS, r, want) if a != b})
        kernels.add((r[0], r[4], r[5], r[6]))
    # the table reaches every family: staged narrow / wide / multi-stream / gate, 1x1 plain / multi-stream, pipelined, overlapped
    assert {(0, 1, 0, 0), (0, 2, 0, 0), (0, 1, 1, 0), (0, 2, 1, 0), (0, 2, 0, 1), (1, 0, 0, 0), (1, 0, 1, 0), (2, 0, 0, 0),
            (3, 0, 0, 0)} <= kernels, kernels


def test_route_reproduces_the_recorded_sweep_digest(lib, golden):
    digest, routed = R.sweep_digest(lib, R.route)
    assert routed == golden["sweep"]["bf16x3_problems"]
    assert digest == golden["sweep"]["sha256"]


def test_fusion_queries_say_what_the_route_says(lib, problems):
    table, sweep = problems
    n_dual = n_gate = 0
    for pr in table + sweep:
        if pr["form"] != "plain" or pr["n"] not in (1, 2, 3, 7, 16, 33):
            continue
        kc, m, oh, ow = pr["kc"], pr["m"], pr["oh"], pr["ow"]
        # dual: the route of the dual problem (a 1x1 data gradient with a derivative source and r) is the 1x1 kernel with four output tiles
        rc, r = R.route(lib, R.problem(pr["n"], kc, oh, ow, m, oh, ow, [0], [0], form="dual"))
        by_route = rc == 0 and (r[0], r[2], r[5]) == (1, 4, 1)
        assert bool(R.dual_ok(lib, pr)) == by_route, pr
        n_dual += by_route
        # gate: the gated problem routes to the wide gate instantiation, and the 1x1 kernel does not take the ungated convolution
        fusable = bool(R.gate_fusable(lib, pr))
        rc, r = R.route(lib, dict(pr, gate=1))
        wide_gate = rc == 0 and (r[0], r[4], r[6]) == (0, 2, 1)
        assert not fusable or wide_gate, pr
        if fusable:
            assert R.route(lib, pr)[1][0] != 1, pr
            n_gate += 1
        if wide_gate and not fusable:  # only the 1x1 kernel's format (one tap, at most 64 input channels) stands in the way
            assert len(pr["dr"]) == 1 and kc <= 64, pr
            even = R.problem(pr["n"], kc, 4, 4, m, 4, 4, [0], [0])
            assert R.route(lib, even)[1][0] == 1, pr
    assert n_dual > 50 and n_gate > 200, (n_dual, n_gate)


def _launch(lib, p, p2, pr):
    ia = ctypes.c_int * len(pr["dr"])
    shape = (pr["n"], pr["kc"], pr["ih"], pr["iw"], pr["m"], pr["oh"], pr["ow"], len(pr["dr"]), ia(*pr["dr"]), ia(*pr["dc"]))
    if pr["form"] == "gate":
        return lib.pg_conv2d_mfma_gate(p, p, None, None, p, *shape, pr["in_act"], pr["gate"] - 1, None, p, None)
    if pr["form"] == "dual":
        return lib.pg_conv2d_mfma_dual(p, p, p, p, pr["n"], pr["kc"], pr["oh"], pr["ow"], pr["m"], p, pr["dact"], p, None)
    res = p if pr["flags"] & R.RES else None
    res2 = None if not pr["flags"] & R.RES2 else (p if pr["flags"] & R.RES2_SAME else p2)
    return lib.pg_conv2d_mfma_ex(p, p, None, res, p, *shape, pr["in_act"], None, 0, pr["out_act"], 2, res2, 0, 0, None)


@_no_gpu
def test_what_the_route_accepts_reaches_the_launch(lib, problems):
    """Fake operands, no device: a launch entry that got past its host side comes back with hipErrorNoDevice. Whatever the route
    accepts must get that far, and what it refuses the launch refuses with the same status."""
    table, sweep = problems
    keep, p = _fake_ptr()
    p2 = ctypes.c_void_p(p.value + 256)
    checked = refused = 0
    for pr in table + [q for q in sweep if R.fmt_of(lib, q) == 2]:
        rc, _ = R.route(lib, pr)
        got = _launch(lib, p, p2, pr)
        if rc == 0:
            assert _reached_launch(lib, got) and got > 0, (pr, got, lib.pg_last_error())
        else:
            assert got == rc, (pr, rc, got, lib.pg_last_error())
            refused += 1
        checked += 1
    assert checked > 4000, (checked, refused)
    del keep


@pytest.mark.parametrize("what,case,want", R.FAMILY_CASES, ids=[c[0] for c in R.FAMILY_CASES])
def test_family_cases_of_the_gpu_tier_reach_their_kernels(lib, what, case, want):
    """tests/test_gpu_ops.py::test_conv_b3_kernel_families runs these; that they land where they say is checked here too."""
    rc, r = R.route(lib, R.family_problem(case))
    got = R.named(r)
    assert rc == 0 and {k: got[k] for k in want} == want, (what, got)


def test_route_export_rejects_bad_arguments(lib):
    out = (ctypes.c_int * len(R.FIELDS))()
    z = (ctypes.c_int * 1)(0)
    args = (2, 64, 8, 8, 64, 8, 8, 1, z, z, 0, 0, 0, 0, 0)
    assert lib.pg_conv_b3_route(*args, out, len(R.FIELDS)) == 0
    assert lib.pg_conv_b3_route(*args, out, len(R.FIELDS) - 1) == -1
    assert lib.pg_conv_b3_route(*args, None, len(R.FIELDS)) == -1
    assert lib.pg_conv_b3_route(2, 64, 8, 8, 64, 8, 8, 0, z, z, 0, 0, 0, 0, 0, out, len(R.FIELDS)) == -1
    assert lib.pg_conv_b3_route(2, 4, 8, 8, 64, 8, 8, 1, z, z, 0, 0, 0, 0, 0, out, len(R.FIELDS)) == -2  # not a bf16x3 shape
    assert b"shape not covered" in lib.pg_last_error()
