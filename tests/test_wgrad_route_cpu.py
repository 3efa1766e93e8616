"""CPU: the weight gradient's route (csrc/conv_wgrad.hip: wgrad_route, exported host-only as pg_conv2d_wgrad_route) and the case
table of tests/_wgrad_cases.py.

  * every case lands on the family and instantiation its entry names, for both input kinds and with and without the bias row;
  * the float64 reference of the table agrees with float64 autograd through F.conv2d on every case, and the exact inputs keep every
    partial sum below 2^24 (what lets the GPU test demand the reference bit for bit);
  * closure: a sweep of random problems (the generator of the forward route's sweep, four seeds, both bias flags) reaches no kernel
    instantiation the table has no case for, and every route it gives fits the workspace, the row cap and the family's LDS limit;
  * the routes of every convolution of the eight bench workloads are the ones recorded in tests/golden/wgrad_routes.json."""

import json
import os

import pytest
import torch
import torch.nn.functional as F

import _conv_b3_routes as R
import _util
import _wgrad_cases as W


@pytest.mark.parametrize("case", W.CASES, ids=lambda c: c.name)
def test_case_lands_where_its_entry_says(lib, case):
    for kind in W.KINDS:
        r = W.route(lib, case, kind)
        assert not W.route_problems(case, r, kind), (case.name, kind, W.route_problems(case, r, kind), r)
        nb = W.route(lib, case, kind, bias=False)  # db = NULL: the same kernel, a smaller reduction
        assert {k: v for k, v in nb.items() if k != "red_grid"} == {k: v for k, v in r.items() if k != "red_grid"}, case.name
        t = len(W.taps(case))
        assert r["red_grid"] == -(-(case.cout * case.cin * t + case.cout) // 64), r
        assert nb["red_grid"] == -(-(case.cout * case.cin * t) // 64), nb
        assert W.route(lib, case, kind) == r


def test_case_table_covers_what_it_is_for(lib):
    rts = {c.name: W.route(lib, c) for c in W.CASES}
    fam = lambda f: [c for c in W.CASES if c.family == f]  # noqa: E731
    assert {c.family for c in W.CASES} == set(W.FAMILIES)
    # half pixel blocks on both tiled bf16x3 kernels
    for f in ("x-copy", "shifted-dy"):
        assert {12, 20, 28} <= {c.ow for c in fam(f)}, f
    # the ring: one image in four segments that start mid-image, an odd number of images, whole-image units plus segments
    assert {1, 3, 20} <= {c.n for c in fam("ring")}
    assert any(c.n == 1 and rts[c.name]["nseg"] == 4 for c in fam("ring"))
    # the generic kernel's tap passes, both staging paths, one and two ci tiles, IH != OH
    gen = fam("generic")
    assert {1, 2, 3, 4, 5, 9, 25, 49} <= {len(W.taps(c)) for c in gen}
    assert any(len(W.taps(c)) == 49 and c.cin == 8 for c in gen)
    assert {(c.inst[1], c.inst[2]) for c in gen} == {(1, 0), (1, 1), (2, 0), (2, 1)}
    assert any(c.oh == c.ih + 1 for c in gen) and any(c.oh == c.ih - 2 for c in gen)
    assert any((c.oh * c.ow) % 4 for c in gen if len(W.taps(c)) == 1)
    assert {"x", "dy", "xdy"} <= {c.mis for c in W.CASES}
    # tiles: one per image, and a ragged last row tile
    assert any(r["tiles_per_img"] == 1 for r in rts.values())
    assert any(r["TR"] > 1 and BY[n].oh % r["TR"] for n, r in rts.items() if r["tiles_per_img"] > 1)
    # the reduction's loop: 1 row, a count that is no multiple of 4, 32 < G < 64 with a remainder, the cap
    gs = {r["G"] for r in rts.values()}
    assert 1 in gs and any(g % 4 for g in gs if g > 4) and any(32 < g < 64 and g % 4 for g in gs)
    capped = {W.FAMILIES[r["family"]] for n, r in rts.items() if r["G"] < min(r["total"], 10 ** 9) and n.startswith("rows-cap")}
    assert capped == set(W.FAMILIES), capped


BY = W.BY_NAME


@pytest.mark.parametrize("case", W.CASES, ids=lambda c: c.name)
def test_reference_agrees_with_float64_autograd(case):
    c = case
    active = torch.zeros(c.kh, c.kw, dtype=torch.bool)
    for _, _, u, v in W.taps(c):
        active[u, v] = True
    for kind in W.KINDS:
        x, dy = W.inputs(c.name, kind)
        act = W.in_act(c, kind)
        dw, db = W.reference(c.name, kind)
        w = torch.zeros(c.cout, c.cin, c.kh, c.kw, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(c.cout, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(W.activation64(x, act), w, b, padding=(c.ph, c.pw))[:, :, :c.oh, :c.ow]
        y.backward(dy.double())
        want = w.grad * active
        scale = float(want.abs().max().clamp_min(1.0))
        assert float((dw - want).abs().max()) <= 1e-12 * scale, (c.name, kind)
        assert float((db - b.grad).abs().max()) <= 1e-12 * float(b.grad.abs().max().clamp_min(1.0)), (c.name, kind)
        assert bool((dw[:, :, ~active] == 0).all())
        if kind == "exact":
            assert act in (0, 1) and bool((x == x.round()).all()) and bool((dy == dy.round()).all())
            assert float(x.abs().max()) <= 8 and float(dy.abs().max()) <= 4
            assert 0.15 < float((dy != 0).float().mean()) < 0.35, c.name
            bw, bb = W.reference_of(x, dy, c, act, absolute=True)  # sum |dy| |x| per output element bounds every partial sum
            assert float(bw.max()) + 3 < 2 ** 24 and float(bb.max()) + 3 < 2 ** 24, (c.name, float(bw.max()))
            assert bool((dw == dw.round()).all()) and bool((dw.float().double() == dw).all())


def _sweep(lib):
    """(problem, flags, status, route) over the random problems of the forward route's sweep, each as a weight-gradient problem with
    and without the bias row; a single tap is routed both as a 1x1 filter and as one tap of a 3x3."""
    for seed in range(4):
        for pr in R.random_problems(seed):
            hr, hc = max(pr["dr"]) - min(pr["dr"]), max(pr["dc"]) - min(pr["dc"])
            filters = [(hr + 1, hc + 1)] + ([(3, 3)] if len(pr["dr"]) == 1 else [])
            for kh, kw in filters:
                for flags in (0, W.HAS_BIAS):
                    args = (pr["n"], pr["kc"], pr["ih"], pr["iw"], pr["m"], pr["oh"], pr["ow"], kh, kw, pr["dr"], pr["dc"])
                    rc, r = W.route_problem(lib, *args, act=0, flags=flags)
                    yield args, flags, rc, r


def test_sweep_reaches_no_kernel_without_a_case(lib):
    covered = {(c.family,) + c.inst for c in W.CASES}
    seen, routed, refused = {}, 0, 0
    for args, flags, rc, r in _sweep(lib):
        if rc != 0:
            assert rc == -2 and (b"LDS" in lib.pg_last_error()), (args, rc, lib.pg_last_error())  # PG_ESHAPE: too wide for any kernel
            refused += 1
            continue
        routed += 1
        n, cin, ih, iw, cout, oh, ow, kh, kw, dr, dc = args
        t = len(dr)
        what = (args, flags, r)
        key = W.key_of(r)
        seen.setdefault(key, args)
        stride = cout * cin * t + cout
        assert 1 <= r["G"] <= r["max_rows"] and r["G"] == r["grid_x"], what
        assert r["G"] * stride <= lib.pg_conv2d_wgrad_workspace_floats(cout, cin, t), what
        assert 0 <= r["lds_bytes"] <= W.LDS_LIMIT[key[0]], what
        assert r["block"] in (256, 512) and r["grid_y"] >= 1 and r["grid_z"] >= 1, what
        assert r["red_grid"] == -(-(cout * cin * t + (cout if flags & W.HAS_BIAS else 0)) // 64), what
        if key[0] != "1x1":
            assert r["G"] <= r["total"], what  # no workgroup without a unit of work: every partial row is written
    assert routed > 20000 and refused < routed // 4, (routed, refused)  # (rows of 128 to 300 pixels with wide halos are refused)
    missing = {k: v for k, v in seen.items() if k not in covered}
    assert not missing, f"kernels the sweep reaches and no case covers: {missing}"
    assert {k[0] for k in seen} == set(W.FAMILIES)


def test_bench_workload_routes_match_the_golden_table(lib):
    with open(os.path.join(_util.GOLDEN_DIR, "wgrad_routes.json")) as f:
        gold = json.load(f)
    assert gold["fields"] == W.FIELDS and gold["families"] == list(W.FAMILIES)
    got = W.bench_routes(lib)
    assert len(got) == len(gold["routes"]) > 100
    diff = [(g[0], dict(zip(W.FIELDS, g[2])), dict(zip(W.FIELDS, w[2]))) for g, w in zip(got, gold["routes"]) if g != w]
    assert not diff, diff[:4]


def test_route_argument_checks(lib):
    from pytorch_generative_amd import _lib

    z, out = _lib.int_array([0]), _lib.int_array([7] * (len(W.FIELDS) + 1))
    ok = (2, 32, 8, 8, 32, 8, 8, 1, 1, 1, z, z, 0, 0)
    assert lib.pg_conv2d_wgrad_route(*ok, out, len(W.FIELDS)) == 0 and out[len(W.FIELDS)] == 7
    out = _lib.int_array([7] * len(W.FIELDS))
    assert lib.pg_conv2d_wgrad_route(*ok, out, len(W.FIELDS) - 1) == -1 and list(out) == [7] * len(W.FIELDS)
    assert lib.pg_conv2d_wgrad_route(*ok, None, len(W.FIELDS)) == -1
    assert lib.pg_conv2d_wgrad_route(2, 32, 8, 8, 32, 8, 8, 1, 1, 0, z, z, 0, 0, out, len(W.FIELDS)) == -2   # T = 0
    assert lib.pg_conv2d_wgrad_route(2, 32, 8, 8, 32, 8, 8, 1, 1, 65, z, z, 0, 0, out, len(W.FIELDS)) == -2  # T > PG_MAX_TAPS
    assert lib.pg_conv2d_wgrad_route(0, 32, 8, 8, 32, 8, 8, 1, 1, 1, z, z, 0, 0, out, len(W.FIELDS)) == -1
    assert lib.pg_conv2d_wgrad_route(2, 32, 8, 8, 32, 8, 8, 1, 1, 1, z, z, 4, 0, out, len(W.FIELDS)) == -1   # bad activation
    assert list(out) == [7] * len(W.FIELDS)
    # a row no kernel's LDS holds: the status and the message of the launch itself
    rc, _ = W.route_problem(lib, 1, 8, 4, 4096, 8, 4, 4096, 3, 3, [-1, 0, 1], [-1, 0, 1])
    assert rc == -2 and b"too wide for LDS" in lib.pg_last_error()
