"""GPU: every kernel family, instantiation and epilogue form of the forward / data-gradient convolution against a plain float64
reference, at the cases of tests/_conv_cases.py, called through the C ABI (pg_conv2d_mfma_ex, pg_conv2d_mfma_gate,
pg_conv2d_mfma_dual, pg_conv2d_taps) so that the buffers and the pointers are the test's own.

Per case and input kind (int / x3 / w3 / x2w2: exact in fp32 in any summation order; random: seeded normals):
  * the weights are packed by pg_pack_conv_weight_frag (gate cases: PG_CONV_FMT_B3_GATE; tap cases: pg_pack_conv_weight) into a
    NaN-filled buffer; one case per family also packs through pg_pack_conv_weight_frag2 and must get the same bits;
  * the route is asked first (pg_conv_b3_route): the case fails if its launch is not the instantiation its entry names
    (tests/test_conv_cases_cpu.py checks the same without a GPU);
  * every output (out, gate_out, out2) is a view inside a larger buffer: the view is prefilled with NaN (a pixel nobody writes makes
    the result non-finite), a 1024-float sentinel band in front of and behind it must come back unchanged; every input is its own
    allocation (a PG_GUARD=1 run then catches reads past the end);
  * a batch-strided residual is a channel slice of a tensor twice as wide whose other channels hold NaN; "the same residual twice"
    passes one pointer twice; a misaligned `in` sits 4 bytes into its buffer;
  * exact kinds: `out` (and `out2` of the dual form) EQUAL the float64 reference — a dropped, swapped or mis-indexed bf16 piece, tap
    slot, K group or lane half is at least one unit per affected product; gate_out, not an exact function, is compared with the
    random kind's tolerance against float64 computed from the exact `out`. Random kind: `_util.GradReport` with the project's
    tolerance and floor, plus the 1e-4 max-norm gate;
  * a second call into fresh buffers returns the same bits (no family uses atomics); the plain form is also called with one fused
    residual: equal to the unfused result plus the residual in the exact kinds, within the tolerance in the random kind.
PG_FAMILY_REPORT=<file> appends one JSON line per case and kind (the source of profiles/conv_families_parity.json); the random kind's
line also records the error of a float32 torch-CPU convolution of the same inputs against the same reference."""

import json
import os

import pytest
import torch

import _conv_b3_routes as R
import _conv_cases as V
import _util

pytestmark = pytest.mark.gpu

TOL = 1e-4
BAND = 1024
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from pytorch_generative_amd import _lib

    _lib.load()  # fail loudly if the extension is missing
    return torch.device("cuda:0")


def _place(t, dev, misaligned=False):
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


class _Out:
    """An output view of `shape` prefilled with NaN between two sentinel bands."""

    def __init__(self, shape, dev):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * BAND,), SENTINEL, device=dev)
        self.view = self.buf[BAND:BAND + n].view(shape)
        self.view.fill_(float("nan"))
        self.n = n
        assert self.view.data_ptr() % 16 == 0

    def bands_ok(self):
        return bool((self.buf[:BAND] == SENTINEL).all()) and bool((self.buf[BAND + self.n:] == SENTINEL).all())


def _sync(what):
    """Wait for the device; a HIP error (a fault in a kernel) ends the whole run: nothing more is started on a GPU that faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{what}: the GPU reported an error, no further test is run: {e}", returncode=3)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _pack(lib, dev, c, w_dev, fmt):
    """The case's weights in the format its launch reads (a NaN-filled buffer: the pack writes all of it)."""
    from pytorch_generative_amd import _lib

    cout, cin = w_dev.shape[:2]
    t = len(c.taps)
    u, v = _lib.int_array([a[2] for a in c.taps]), _lib.int_array([a[3] for a in c.taps])
    transpose = int(c.orient == "dgrad")
    if c.backend == "taps":
        b_pad = lib.pg_conv_b_pad(c.m)
        wpk = torch.full((c.k * t * b_pad,), float("nan"), device=dev)
        assert lib.pg_packed_weight_floats(c.k, t, c.m) == wpk.numel()
        _lib.check(lib.pg_pack_conv_weight(w_dev.data_ptr(), wpk.data_ptr(), cout, cin, c.kh, c.kw, t, u, v, transpose, b_pad, None),
                   f"pg_pack_conv_weight({c.name})")
        return wpk
    wfrag = torch.full((lib.pg_conv_frag_floats(c.k, c.m, t, fmt),), float("nan"), device=dev)
    _lib.check(lib.pg_pack_conv_weight_frag(w_dev.data_ptr(), wfrag.data_ptr(), cout, cin, c.kh, c.kw, t, u, v, transpose, fmt, None),
               f"pg_pack_conv_weight_frag({c.name})")
    if c.name in V.PACK2_CASES:
        # both orientations in one launch: this case's side must hold the same bits, the other side those of its own single pack
        hr = max(a[0] for a in c.taps) - min(a[0] for a in c.taps)
        hc = max(a[1] for a in c.taps) - min(a[1] for a in c.taps)
        ofmt = lib.pg_conv_mfma_supported(c.m, c.k, t, c.ih, c.iw, c.ow, hr, hc)
        assert ofmt in (V.FMT_F32, V.FMT_B3), (c.name, ofmt)
        mine = torch.full_like(wfrag, float("nan"))
        other = torch.full((lib.pg_conv_frag_floats(c.m, c.k, t, ofmt),), float("nan"), device=dev)
        single = torch.full_like(other, float("nan"))
        fwd, dgr = (mine, other) if not transpose else (other, mine)
        _lib.check(lib.pg_pack_conv_weight_frag2(w_dev.data_ptr(), fwd.data_ptr(), dgr.data_ptr(), cout, cin, c.kh, c.kw, t, u, v,
                                                 ofmt if transpose else fmt, fmt if transpose else ofmt, None), "pg_pack_conv_weight_frag2")
        _lib.check(lib.pg_pack_conv_weight_frag(w_dev.data_ptr(), single.data_ptr(), cout, cin, c.kh, c.kw, t, u, v, 1 - transpose, ofmt,
                                                None), "pg_pack_conv_weight_frag")
        _sync(c.name + " (pack)")
        assert torch.equal(mine.view(torch.int32), wfrag.view(torch.int32)), c.name + ": frag2 packs other bits than frag"
        assert torch.equal(other.view(torch.int32), single.view(torch.int32)), c.name + ": frag2's other orientation differs"
    _sync(c.name + " (pack)")
    assert bool(torch.isfinite(wfrag).all()), c.name + ": the pack left part of the fragment buffer unwritten"
    return wfrag


class _Operands:
    """The device operands of (case, kind), each its own allocation."""

    def __init__(self, lib, dev, c, kind):
        d = V.inputs(c.name, kind)
        self.keep = []
        self.x, owner = _place(d["x"], dev, "in" in c.mis)
        self.keep.append(owner)
        self.w = d["w"].to(dev)
        fmt = V.FMT_B3_GATE if c.form == "gate" else V.FMT_OF_BACKEND[c.backend]
        self.wpk = _pack(lib, dev, c, self.w, fmt)
        self.bias = None if d["bias"] is None else d["bias"].to(dev)
        self.res, self.res2, self.dact_src = d["res"].to(dev), d["res2"].to(dev), d["dact_src"].to(dev)
        self.gate_res, self.r = d["gate_res"].to(dev), d["r"].to(dev)
        # the batch-strided residual: channels [M / 2, M / 2 + M) of a tensor twice as wide, NaN elsewhere
        self.wide = torch.full((c.n, 2 * c.m, c.oh, c.ow), float("nan"), device=dev)
        self.wide[:, c.m // 2:c.m // 2 + c.m] = self.res
        self.res_slice = self.wide[:, c.m // 2:c.m // 2 + c.m]


def _call(lib, dev, c, kind, ops, fused_res=False):
    """One launch of the case into fresh guarded outputs -> ({name: tensor}, bands untouched)."""
    from pytorch_generative_amd import _lib

    a = V.acts_of(c, kind)
    ia = _lib.int_array
    dr, dc = ia([t[0] for t in c.taps]), ia([t[1] for t in c.taps])
    shape = (c.n, c.k, c.ih, c.iw, c.m, c.oh, c.ow, len(c.taps), dr, dc)
    flags = V.FORM_FLAGS[c.form]
    outs = {"out": _Out((c.n, c.m, c.oh, c.ow), dev)}
    out = outs["out"].view
    if c.form == "gate":
        has_res, has_gate_res = V.gate_operands(c, kind)
        outs["gate_out"] = _Out((c.n, c.m // 2, c.oh, c.ow), dev)
        rc = lib.pg_conv2d_mfma_gate(ops.x.data_ptr(), ops.wpk.data_ptr(), _ptr(ops.bias), _ptr(ops.res) if has_res else None,
                                     out.data_ptr(), *shape, a["in_act"], a["gate"], _ptr(ops.gate_res) if has_gate_res else None,
                                     outs["gate_out"].view.data_ptr(), None)
    elif c.form == "dual":
        outs["out2"] = _Out((c.n, c.m, c.oh, c.ow), dev)
        rc = lib.pg_conv2d_mfma_dual(ops.x.data_ptr(), ops.wpk.data_ptr(), out.data_ptr(), outs["out2"].view.data_ptr(), c.n, c.k, c.oh,
                                     c.ow, c.m, ops.dact_src.data_ptr(), a["dact"], ops.r.data_ptr(), None)
    else:
        res = ops.res_slice if flags & R.RES_STRIDED else (ops.res if (flags & R.RES or fused_res) else None)
        res2 = None if not flags & R.RES2 else (res if flags & R.RES2_SAME else ops.res2)
        res_bs = ops.wide.stride(0) if flags & R.RES_STRIDED else 0
        dsrc = ops.dact_src if flags & R.DACT_SRC else None
        if c.backend == "taps":
            rc = lib.pg_conv2d_taps(ops.x.data_ptr(), ops.wpk.data_ptr(), _ptr(ops.bias), _ptr(res), out.data_ptr(), *shape,
                                    a["in_act"], _ptr(dsrc), a["dact"], None)
        else:
            rc = lib.pg_conv2d_mfma_ex(ops.x.data_ptr(), ops.wpk.data_ptr(), _ptr(ops.bias), _ptr(res), out.data_ptr(), *shape,
                                       a["in_act"], _ptr(dsrc), a["dact"], a["out_act"], V.FMT_OF_BACKEND[c.backend], _ptr(res2),
                                       res_bs, 0, None)
    if rc > 0:
        pytest.exit(f"launch of {c.name} ({kind}): HIP error {rc} ({lib.pg_last_error()}), no further test is run", returncode=3)
    _lib.check(rc, f"launch of {c.name} ({kind})")
    _sync(f"{c.name} ({kind})")
    return {k: o.view for k, o in outs.items()}, all(o.bands_ok() for o in outs.values())


@pytest.mark.parametrize("kind", V.KINDS)
@pytest.mark.parametrize("case", V.CASES, ids=lambda c: c.name)
def test_family_against_float64(dev, lib, case, kind):
    c = case
    a = V.acts_of(c, kind)
    if c.backend == "b3":
        r = V.route(lib, c, kind)
        key = V.key_of(r)
        bad = V.route_problems(c, r, kind)
    else:
        r = {k: 0 for k in R.FIELDS}
        key, bad = (c.backend,), []
        assert V.fmt_of(lib, c) == V.FMT_OF_BACKEND[c.backend], c.name
    print(f"[family] {c.name} ({kind}, act {V.ACTS[a['in_act']]}): {key} grid {r['grid_x']}x{r['grid_y']}x1 block {r['block']} "
          f"lds {r['lds_bytes']} TR {r['TR']} tiles {r['tiles_per_img']} form {c.form} {c.orient}")
    assert not bad, f"{c.name} does not run what its entry says: {bad}"
    what = f"{c.name} ({kind}, {key})"

    ops = _Operands(lib, dev, c, kind)
    got, bands = _call(lib, dev, c, kind, ops)
    got2, bands2 = _call(lib, dev, c, kind, ops)
    assert bands and bands2, what + ": a sentinel band around an output was written"
    for name, t in got.items():
        assert bool(torch.isfinite(t).all()), f"{what}: {name} is not finite (a pixel nobody wrote, or an operand read outside its slice)"
    ref = V.reference(c.name, kind)
    assert set(got) == set(ref)

    rep = _util.GradReport(what)
    for name in sorted(got):
        rep.add(name, got[name], ref[name])
    extra = {}
    fused = None
    if c.form == "plain":  # the same launch with one fused residual
        fused, bands_f = _call(lib, dev, c, kind, ops, fused_res=True)
        assert bands_f, what + ": a sentinel band was written by the launch with a residual"
        rep.add("out with a fused residual", fused["out"], V.reference(c.name, kind, True)["out"])
    if kind == "random":
        d = V.inputs(c.name, kind)
        cpu32 = V.torch_reference(c, kind, d, dtype=torch.float32)
        extra["torch_cpu_fp32_max_norm_err"] = {k: _util.rel_err(cpu32[k], ref[k]) for k in sorted(ref)}
    _report(c, kind, key, r, rep.rows, extra)

    if kind == "random":
        rep.finish()
        for name in got:
            _util.assert_close(got[name], ref[name], TOL, f"{what} {name}")
    else:
        for name in sorted(got):
            if name == "gate_out":
                continue
            g, w = got[name].cpu(), ref[name].float()
            wrong = int((g != w).sum())
            assert torch.equal(g, w), (f"{what}: {wrong} of {w.numel()} entries of {name} differ, largest difference "
                                       f"{float((g.double() - ref[name]).abs().max())} ({V.UNIT[kind]} = one unit)")
        if fused is not None:
            want = (got["out"].cpu().double() + V.inputs(c.name, kind)["res"].double()).float()
            assert torch.equal(fused["out"].cpu(), want), \
                f"{what}: the fused residual differs from the unfused result plus the residual by up to " \
                f"{float((fused['out'].cpu().double() - want.double()).abs().max())}"
        rep.finish()  # gate_out (from the exact out) within the random kind's tolerance; the rest is zero
    for name in got:
        assert torch.equal(got2[name], got[name]), f"{what}: two runs differ in {name}"


def _report(c, kind, key, r, rows, extra):
    path = os.environ.get("PG_FAMILY_REPORT")
    if not path:
        return
    a = V.acts_of(c, kind)
    rec = {"case": c.name, "kind": kind, "backend": c.backend, "orient": c.orient, "form": c.form, "family": key[0],
           "instantiation": dict(zip(("MT", "CG", "MS", "GT", "gelu", "two_tiles", "NT"), key[1:])),
           "acts": {k: V.ACTS[a[k]] for k in ("in_act", "out_act", "dact")},
           "route": {k: r[k] for k in ("grid_x", "grid_y", "block", "lds_bytes", "TR", "tiles_per_img", "CIB", "ksteps")}}
    for name, mn, el, _ in rows:
        rec[name] = {"max_norm_err": mn, "elementwise_ratio": el}
    rec.update(extra)
    with open(path, "a") as f:
        f.write(json.dumps(rec) + "\n")
