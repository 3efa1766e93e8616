"""GPU: the three kernel families of causal softmax attention against float64, at the shapes of tests/_attn_cases.py.

  valu  csrc/attention.hip row-owner kernels beyond L = 63: a second 64-row block per wave, odd block counts, several LDS
        tiles, several workgroups per (n, head), every Cfg<DK, DV> instantiation
  m44   csrc/attention_mfma.hip (d_k = d_v = 4) where its kernels run out of LDS one by one, so that one forward / backward
        mixes matrix-core and VALU kernels: lse2 (log2 domain, 1e30 for an empty row) and delta cross between the families
  k4    csrc/attention_k4.hip: every instantiation row, one key tile, the 64-row blocks (QB = 4) of >= 3072 units, and
        scores that step up by ~19 log2 units on its tile boundaries
Every case first asks `ops.attention_route` where its launches go and fails if that is not the family its entry names
(tests/test_attn_route_cpu.py checks the same without a GPU). Then output, dQ, dK, dV against float64
`oracle.ops.causal_attention_core` with the fused-backward switch on and off: the suite's 1e-4 max-norm gate on the output,
`_util.GradReport` (default tolerance and floor) on the three gradients, a strict mask's first row exactly zero, everything
finite; with the switch off a second run of the VALU and k4 families must return the same bits. The output's element-wise
ratio (same gate as the gradients') is printed, not asserted."""

import pytest
import torch

import _attn_cases as A
import _util

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from pytorch_generative_amd import _lib

    _lib.load()  # fail loudly if the extension is missing
    return torch.device("cuda:0")


def _run(dev, c, q, kv, d_o):
    """(o, dq, dk, dv) of one forward + backward on the device, through the op the case names."""
    from pytorch_generative_amd import ops

    e, v = c.heads * c.dk, c.heads * c.dv
    if c.merged:  # q, k, v views of one tensor: batch strides differ from the plane sizes
        t = torch.cat((q, kv), dim=1).to(dev).requires_grad_(True)
        o = ops.causal_attention_qkv(t, c.heads, e, v, c.strict)
        o.backward(d_o.to(dev))
        g = t.grad
        return o.detach(), g[:, :e], g[:, e:2 * e], g[:, 2 * e:]
    qg, kvg = q.to(dev).requires_grad_(True), kv.to(dev).requires_grad_(True)
    o = ops.causal_attention(qg, kvg, c.heads, e, v, c.strict)
    o.backward(d_o.to(dev))
    return o.detach(), qg.grad, kvg.grad[:, :e], kvg.grad[:, e:]


@pytest.mark.parametrize("deterministic", [False, True], ids=["fused-bwd", "two-kernel-bwd"])
@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.name)
def test_family_against_float64(dev, case, deterministic):
    from pytorch_generative_amd import ops

    c = case
    q, kv, d_o = A.inputs(c.name)
    o_ref, dq_ref, dk_ref, dv_ref = A.reference(c.name)
    was = ops.set_deterministic(deterministic)
    try:
        rts = A.routes(c)
        bad = A.route_problems(c, rts, fused_on=not deterministic)
        fams = "/".join(r["family"] for r in rts)
        print(f"[family] {c.name}: fwd/dq/dkv/fused on {fams}"
              + "".join(f" {k}<{r['t0']},{r['t1']},{r['qb']}> grid {r['grid_x']} tiles {r['tiles']}" for k, r in zip(A.KERNELS, rts)
                        if r["family"] not in ("declined", "none")))
        assert not bad, f"{c.name} does not run what its entry says: {bad}"
        got = _run(dev, c, q, kv, d_o)
        again = _run(dev, c, q, kv, d_o) if deterministic and A.family_of(c) in ("valu", "k4") else None
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(was)
    what = f"{c.name} ({'two-kernel' if deterministic else 'fused'} backward, {fams})"
    o, dq, dk, dv = (t.cpu() for t in got)
    assert all(bool(torch.isfinite(t).all()) for t in (o, dq, dk, dv)), what + ": non-finite values"
    out = _util.GradReport(what + " output")  # measures only: the output's gate is the max-norm below
    out.add("o", o, o_ref)
    print(f"[output] {what}: max-norm err {out.rows[0][1]:.3e}, element-wise ratio {out.rows[0][2]:.3f} (not asserted)")
    _util.assert_close(o, o_ref, TOL, what + " output")
    if c.strict:  # the row with no allowed key is exactly zero
        assert torch.equal(o[:, :, 0, 0], torch.zeros(c.n, c.heads * c.dv)), what
    rep = _util.GradReport(what)
    rep.add("dq", dq, dq_ref)
    rep.add("dk", dk, dk_ref)
    rep.add("dv", dv, dv_ref)
    _report(c, deterministic, fams, out.rows[0], rep.rows)
    rep.finish()
    if again is not None:
        for name, a, b in zip(("output", "dq", "dk", "dv"), got, again):
            assert torch.equal(a, b), f"{what}: {name} differs between two runs"


def _report(c, deterministic, fams, out_row, grad_rows):
    """PG_FAMILY_REPORT=<file>: one JSON line per case and mode with the figures of all four tensors (the source of
    profiles/attention_families_parity.json)."""
    import json
    import os

    path = os.environ.get("PG_FAMILY_REPORT")
    if not path:
        return
    rec = {"case": c.name, "family": A.family_of(c), "backward": "two-kernel" if deterministic else "fused", "routes": fams,
           "boost": bool(c.boost)}
    for name, mn, el, _ in [out_row] + grad_rows:
        rec[name] = {"max_norm_err": mn, "elementwise_ratio": el}
    with open(path, "a") as f:
        f.write(json.dumps(rec) + "\n")
