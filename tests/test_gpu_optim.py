"""GPU: the optimiser half of the step (csrc/optim.hip through optim.FlatAdam) against a float64 restatement.

FlatAdam over plain nn.Parameters, a prepared gradient stream written straight into `p._pg_grad`, `step()`, and the
same sequence through `clip_grad_norm_` + `torch.optim.Adam` in float64 on the CPU (tests/_optim_ref.py). Asserted
per step: `grad_norm()` at 1e-4. At steps 1, 2, 10, K/2 and K: parameters and both moments (read through
`state_dict()`) within `4 e_ref + 1e-7 max|x|`, e_ref = distance of the float32 restatement to float64 at that step;
`current_lr()` within K 2^-23 relative of fp32(lr) decay^K (the decay constant is rounded once to fp32 and every
product once); the step counter. One JSON line per case (`[optim parity]`, appended to PG_PARITY_REPORT when set).
Then the exactness properties: power-of-two pre-scale, zero gradients, padding slots, run-to-run bit identity."""

import json
import os

import pytest
import torch

import _optim_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NORM_TOL = 1e-4

CASES = ([(lay, reg, 200) for lay in R.SMALL for reg in R.REGIMES]
         + [("n4099", reg, 300) for reg in R.REGIMES]
         + [("mid", reg, 40) for reg in ("clip_all", "clip_some_decay", "prescale_decay", "prescale_clip")]
         + [("big", reg, 16) for reg in ("clip_all", "clip_some_decay", "prescale_decay", "prescale_clip")])


def _build(sc):
    """FlatAdam over fresh GPU parameters of the scenario (followers declared), regime's lr / decay, max_norm of step 0."""
    from pytorch_generative_amd import optim

    params = [torch.nn.Parameter(p.to(DEV)) for p in sc.init_params()]
    for p, f in zip(params, sc.follows):
        if f is not None:
            p._pg_follows = params[f]
    opt = optim.FlatAdam(params, lr=sc.lr, betas=R.BETAS, eps=R.EPS, max_norm=sc.max_norm[0], lr_decay=sc.decay)
    return params, opt


def _read(params, opt):
    sd = opt.state_dict()
    return {"params": [p.detach().cpu() for p in params],
            "exp_avg": [sd["state"][i]["exp_avg"].cpu() for i in range(len(params))],
            "exp_avg_sq": [sd["state"][i]["exp_avg_sq"].cpu() for i in range(len(params))],
            "lr": opt.current_lr(), "step": float(sd["state"][0]["step"])}


def _play(sc, params, opt, on_mark=None, marks=()):
    """Runs the scenario on the GPU; returns the per-step grad_norm() as floats."""
    norms = []
    for k in range(sc.K):
        if k == 0 or sc.max_norm[k] != sc.max_norm[k - 1]:
            opt.set_max_norm(sc.max_norm[k])
        if k == 0 or sc.prescale[k] != sc.prescale[k - 1]:
            opt.set_grad_prescale(sc.prescale[k])
        for p, g in zip(params, sc.grads(k)):
            p._pg_grad.copy_(g.to(DEV))
        opt.step()
        norms.append(float(opt.grad_norm()))
        if k + 1 in marks:
            on_mark(k + 1)
    return norms


def _padding_mask(params, opt):
    used = torch.zeros(opt._numel, dtype=torch.bool)
    for p, o in zip(params, opt._offsets):
        used[o:o + p.numel()] = True
    return ~used


def _assert_padding_zero(params, opt, what):
    pad = _padding_mask(params, opt).to(DEV)
    for name in ("flat_param", "flat_grad", "exp_avg", "exp_avg_sq"):
        buf = getattr(opt, name)
        assert buf.numel() == opt._numel
        if bool(pad.any()):
            assert bool((buf[pad] == 0).all()), f"{what}: padding slots of {name} are not exactly 0"


@pytest.mark.parametrize("layout,regime,K", CASES, ids=[f"{a}-{b}" for a, b, _ in CASES])
def test_flat_adam_against_float64(layout, regime, K):
    sc = R.Scenario(layout, regime, K)
    n64, s64 = R.run(sc, torch.float64)
    _, s32 = R.run(sc, torch.float32)
    params, opt = _build(sc)
    if layout == "follows":  # the declared pair really is back to back, and the 9-element follower is padded
        assert opt._offsets == [0, 8, 20] and opt._numel == 28
    if layout == "ragged":
        assert opt._offsets == [0, 8, 24, 28] and opt._numel == 28 + 2112
    got = {}
    gn = _play(sc, params, opt, on_mark=lambda k: got.__setitem__(k, _read(params, opt)), marks=set(sc.checkpoints()))
    torch.cuda.synchronize()

    norm_err = max((abs(a - b) / b if b > 0 else abs(a)) for a, b in zip(gn, n64))
    rec = {"case": f"{layout}/{regime}", "K": K, "numel": R.numel(layout), "clipped_steps": R.clipped_steps(sc, n64),
           "grad_norm_worst_rel_err": norm_err, "checkpoints": {}}
    fp32_lr, failures = float(torch.tensor(sc.lr, dtype=torch.float32)), []
    # largest gradient entry that entered the moments so far, after pre-scale and clip (float64 restatement)
    geff, run_max = [], 0.0
    for k in range(sc.K):
        coef = 1.0 if sc.max_norm[k] is None else min(1.0, sc.max_norm[k] / (n64[k] + 1e-6))
        run_max = max(run_max, R.max_abs(sc.grads(k)) * sc.prescale[k] * coef)
        geff.append(run_max)
    for k in sc.checkpoints():
        row = {}
        for key in ("params", "exp_avg", "exp_avg_sq"):
            e_ref, bound = R.e_ref(s32[k], s64[k], key), R.bound(s32[k], s64[k], key)
            # The moments are signed running sums: with 1-5 elements exp_avg can sit near 0 at a checkpoint while every
            # term it was summed from was rounded relative to the gradients' size, and e_ref of one to three samples is
            # a noisy estimate. Their absolute floor is therefore 1e-7 of the largest term summed so far (|g| for
            # exp_avg, g^2 for exp_avg_sq), not of the momentary value. The parameters keep the bound as it stands.
            if key == "exp_avg":
                bound = max(bound, 4.0 * e_ref + 1e-7 * geff[k - 1])
            elif key == "exp_avg_sq":
                bound = max(bound, 4.0 * e_ref + 1e-7 * geff[k - 1] ** 2)
            err = R.max_abs_diff(got[k][key], s64[k][key])
            row[key] = {"e_ref": e_ref, "gpu_err": err, "ratio_to_e_ref": (err / e_ref if e_ref else None), "bound": bound}
            if not err <= bound:
                failures.append(f"step {k} {key}: |gpu - f64| {err:.3e} > 4 e_ref + 1e-7 max = {bound:.3e} (e_ref {e_ref:.3e})")
        want_lr = fp32_lr * sc.decay ** k
        drift = abs(got[k]["lr"] - want_lr) / want_lr
        row["lr_rel_drift"], row["lr_bound"] = drift, (k * R.TWO_M23 if sc.decay != 1.0 else 0.0)
        if not drift <= row["lr_bound"]:
            failures.append(f"step {k} lr: relative drift {drift:.3e} > {row['lr_bound']:.3e}")
        if got[k]["step"] != float(k) or float(opt.state_block[0]) != float(sc.K):
            failures.append(f"step counter {got[k]['step']} at step {k}")
        rec["checkpoints"][str(k)] = row
    print("[optim parity] " + json.dumps(rec))
    path = os.environ.get("PG_PARITY_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")
    for k, (a, b) in enumerate(zip(gn, n64)):
        assert abs(a - b) <= NORM_TOL * b, f"step {k + 1}: grad_norm() {a!r} vs float64 {b!r}"
    assert not failures, f"{layout}/{regime}: " + "; ".join(failures)
    _assert_padding_zero(params, opt, f"{layout}/{regime}")


@pytest.mark.parametrize("layout", ["n1", "n5", "ragged", "follows", "mid"])
def test_power_of_two_prescale_is_exact(layout):
    """max_norm unset: gradients x8 with pre-scale 1/8 == gradients x1 with pre-scale 1, bit for bit (coef is exactly 1)."""
    K = 30
    a, b = R.Scenario(layout, "prescale_decay", K), R.Scenario(layout, "prescale_decay", K)
    b.gscale, b.prescale = [1.0] * K, [1.0] * K
    pa, oa = _build(a)
    pb, ob = _build(b)
    na, nb = _play(a, pa, oa), _play(b, pb, ob)
    assert na == nb
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
    assert torch.equal(oa.exp_avg, ob.exp_avg) and torch.equal(oa.exp_avg_sq, ob.exp_avg_sq)
    assert float(oa.state_block[4]) == 0.125 and float(ob.state_block[4]) == 1.0  # coef * pre


@pytest.mark.parametrize("layout", ["n1", "n3", "ragged", "mid"])
def test_zero_gradients_leave_parameters_bit_unchanged(layout):
    sc = R.Scenario(layout, "zeros_only", 10)
    params, opt = _build(sc)
    before = [p.detach().clone() for p in params]
    norms = _play(sc, params, opt)
    assert norms == [0.0] * 10
    for p, q in zip(params, before):
        assert torch.equal(p, q)
    assert float(opt.exp_avg.abs().max()) == 0.0 and float(opt.exp_avg_sq.abs().max()) == 0.0
    assert float(opt.state_block[0]) == 10.0 and float(opt.state_block[4]) == 1.0


def _two_runs(layout, regime, K):
    out = []
    for _ in range(2):
        sc = R.Scenario(layout, regime, K)
        params, opt = _build(sc)
        norms = _play(sc, params, opt)
        torch.cuda.synchronize()
        out.append((norms, [p.detach().clone() for p in params], opt.exp_avg.clone(), opt.exp_avg_sq.clone(), sc))
    return out


def _assert_identical(runs, what):
    (n1, p1, m1, v1, sc), (n2, p2, m2, v2, _) = runs
    assert R.clipped_steps(sc, n1) >= sc.K // 3, "the scenario must clip"
    assert n1 == n2, f"{what}: grad_norm() differs between two identical runs: " + str(
        [(k, a, b) for k, (a, b) in enumerate(zip(n1, n2)) if a != b][:4])
    for a, b in zip(p1, p2):
        assert torch.equal(a, b), f"{what}: parameters differ between two identical runs"
    assert torch.equal(m1, m2) and torch.equal(v1, v2)


@pytest.mark.parametrize("layout", ["n5", "follows"])
def test_single_block_clipping_is_bit_reproducible(layout):
    """Flat buffers of 8 and 28 floats: one block, nothing summed across blocks."""
    _assert_identical(_two_runs(layout, "clip_some_decay", 60), layout)


@pytest.mark.parametrize("regime", ["clip_all", "prescale_clip"])
def test_clipping_is_bit_reproducible_at_three_million_elements(regime):
    """1024 blocks feed the norm here. Their partial sums are stored per block and added in a fixed order by the prepare
    kernel, so with a finite max_norm — where the norm scales every gradient — two identical runs of K = 20 steps
    give the same bits: grad_norm() of every step, parameters, both moments. (One float atomicAdd per block into one
    word, the earlier form, is added in arrival order.) Each run happens once: a comparison of two results."""
    from pytorch_generative_amd import ops

    was = ops.set_deterministic(True)
    try:
        _assert_identical(_two_runs("big", regime, 20), f"big/{regime}")
    finally:
        ops.set_deterministic(was)


def test_measure_grad_norm_equals_the_step_norm():
    """Trainer's skip path reads `measure_grad_norm()` BEFORE stepping: same quantity as the fused norm, pre-scale included."""
    sc = R.Scenario("ragged", "prescale_clip", 6)
    n64, _ = R.run(sc, torch.float64)
    params, opt = _build(sc)
    for k in range(sc.K):
        opt.set_grad_prescale(sc.prescale[k])
        for p, g in zip(params, sc.grads(k)):
            p._pg_grad.copy_(g.to(DEV))
        m = float(opt.measure_grad_norm())
        opt.step()
        assert abs(m - n64[k]) <= NORM_TOL * n64[k] and abs(float(opt.grad_norm()) - m) <= 1e-6 * m
