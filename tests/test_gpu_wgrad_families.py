"""GPU: every kernel family and instantiation of `pg_conv2d_wgrad` against a plain float64 reference, at the cases of
tests/_wgrad_cases.py, called through the C ABI so that the workspace and the pointers are the test's own.

Per case and input kind (exact integers / seeded normals):
  * the route is asked first (`pg_conv2d_wgrad_route`): the case fails if its launch is not the family and instantiation its entry
    names (tests/test_wgrad_route_cpu.py checks the same without a GPU);
  * the workspace is filled with NaN, followed by a 1024-float canary tail: a partial-row slot the reduction reads and no workgroup
    wrote makes the result non-finite (production hands the kernels uninitialised memory), a write past the queried size changes
    the tail;
  * dw and db are prefilled with small integers: the reduction ADDS to them;
  * exact inputs: dw - prefill and db - prefill EQUAL the float64 reference (every product and partial sum is an integer below 2^24,
    so the summation order cannot matter: a dropped, duplicated or shifted pixel, a leaked halo row or a wrong tap slot is an integer
    difference); random inputs: `_util.GradReport` with the project's tolerance and floor, plus the 1e-4 max-norm gate;
  * a run with db = NULL returns the same dw bits, and a second run into fresh buffers returns the same bits (no family uses atomics).
PG_FAMILY_REPORT=<file> appends one JSON line per case and kind (the source of profiles/wgrad_families_parity.json)."""

import json
import os

import pytest
import torch

import _util
import _wgrad_cases as W

pytestmark = pytest.mark.gpu

TOL = 1e-4
TAIL = 1024
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from pytorch_generative_amd import _lib

    _lib.load()  # fail loudly if the extension is missing
    return torch.device("cuda:0")


def _place(t, dev, misaligned):
    """The tensor on the device, 16-byte aligned or (misaligned) 4 bytes into a buffer one float longer. Returns (view, owner)."""
    if not misaligned:
        d = t.to(dev).contiguous()
        assert d.data_ptr() % 16 == 0
        return d, d
    buf = torch.empty(t.numel() + 1, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() == buf.data_ptr() + 4
    return view, buf


def _call(lib, dev, c, act, x, dy, bias):
    """One pg_conv2d_wgrad call into prefilled outputs and a poisoned workspace -> (dw, db or None, tail untouched)."""
    from pytorch_generative_amd import _lib

    t = W.taps(c)
    dw = W.prefill((c.cout, c.cin, c.kh, c.kw)).to(dev)
    db = W.prefill((c.cout,)).to(dev) if bias else None
    need = lib.pg_conv2d_wgrad_workspace_floats(c.cout, c.cin, len(t))
    ws = torch.full((need + TAIL,), float("nan"), device=dev)
    ws[need:] = SENTINEL
    ia = _lib.int_array
    rc = lib.pg_conv2d_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr() if bias else None, c.n, c.cin, c.ih, c.iw,
                             c.cout, c.oh, c.ow, c.kh, c.kw, len(t), ia([a[0] for a in t]), ia([a[1] for a in t]),
                             ia([a[2] for a in t]), ia([a[3] for a in t]), act, ws.data_ptr(), need, None)
    _lib.check(rc, f"pg_conv2d_wgrad({c.name})")
    torch.cuda.synchronize()
    return dw, db, bool((ws[need:] == SENTINEL).all())


@pytest.mark.parametrize("kind", W.KINDS)
@pytest.mark.parametrize("case", W.CASES, ids=lambda c: c.name)
def test_family_against_float64(dev, lib, case, kind):
    c = case
    act = W.in_act(c, kind)
    r = W.route(lib, c, kind)
    key = W.key_of(r)
    print(f"[family] {c.name} ({kind}, act {W.ACTS[act]}): {key} grid {r['grid_x']}x{r['grid_y']}x{r['grid_z']} block {r['block']} "
          f"lds {r['lds_bytes']} G {r['G']} TR {r['TR']} tiles {r['total']} nseg {r['nseg']}")
    bad = W.route_problems(c, r, kind)
    assert not bad, f"{c.name} does not run what its entry says: {bad}"
    assert W.key_of(W.route(lib, c, kind, bias=False)) == key

    x_cpu, dy_cpu = W.inputs(c.name, kind)
    dw_ref, db_ref = W.reference(c.name, kind)
    x, _keep_x = _place(x_cpu, dev, "x" in c.mis)
    dy, _keep_dy = _place(dy_cpu, dev, "dy" in c.mis)
    what = f"{c.name} ({kind}, {key})"

    dw, db, tail_ok = _call(lib, dev, c, act, x, dy, bias=True)
    dw2, db2, tail_ok2 = _call(lib, dev, c, act, x, dy, bias=True)
    dw_nb, _, tail_ok_nb = _call(lib, dev, c, act, x, dy, bias=False)
    assert tail_ok and tail_ok2 and tail_ok_nb, what + ": the workspace was written past the queried size"
    for name, t in (("dw", dw), ("db", db), ("dw without bias", dw_nb)):
        assert bool(torch.isfinite(t).all()), f"{what}: {name} is not finite (a partial-row slot nobody wrote was reduced)"

    got_w = dw.cpu().double() - W.prefill(dw.shape).double()
    got_b = db.cpu().double() - W.prefill(db.shape).double()
    rep = _util.GradReport(what)
    rep.add("dw", got_w, dw_ref)
    rep.add("db", got_b, db_ref)
    _report(c, kind, key, r, rep.rows)
    if kind == "exact":
        wrong = int((got_w.float() != dw_ref.float()).sum())
        assert torch.equal(got_w.float(), dw_ref.float()), \
            f"{what}: {wrong} of {dw_ref.numel()} dw entries differ, largest difference {float((got_w - dw_ref).abs().max())}"
        assert torch.equal(got_b.float(), db_ref.float()), f"{what}: db differs by up to {float((got_b - db_ref).abs().max())}"
        rep.finish()
    else:
        rep.finish()
        _util.assert_close(got_w, dw_ref, TOL, what + " dw")
        _util.assert_close(got_b, db_ref, TOL, what + " db")
    assert torch.equal(dw_nb, dw), what + ": dw differs between db given and db = NULL"
    assert torch.equal(dw2, dw) and torch.equal(db2, db), what + ": two runs differ"


def _report(c, kind, key, r, rows):
    path = os.environ.get("PG_FAMILY_REPORT")
    if not path:
        return
    rec = {"case": c.name, "kind": kind, "family": key[0], "instantiation": list(key[1:]), "act": W.ACTS[W.in_act(c, kind)],
           "route": {k: r[k] for k in ("grid_x", "grid_y", "grid_z", "block", "lds_bytes", "TR", "total", "nseg")}, "G": r["G"]}
    for name, mn, el, _ in rows:
        rec[name] = {"max_norm_err": mn, "elementwise_ratio": el}
    with open(path, "a") as f:
        f.write(json.dumps(rec) + "\n")
