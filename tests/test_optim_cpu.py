"""CPU: the yardstick of tests/test_gpu_optim.py and the Trainer's step / skip decision.

The GPU test holds FlatAdam to `4 e_ref + 1e-7 max|p|` of a float64 restatement, e_ref being the distance of the
SAME restatement in float32 (the reference's own arithmetic). Here e_ref is re-derived for every regime: it must be
non-zero (the bound is not a demand for exact float64 results) and below 1e-2 lr (an error of 1 % of one step, in
one step out of K, would already exceed it: the bound is not vacuous)."""

import math

import pytest
import torch

import _optim_ref as R


@pytest.mark.parametrize("regime", R.REGIMES)
def test_e_ref_is_neither_zero_nor_loose(regime):
    sc = R.Scenario("n4099", regime, 300)
    n64, s64 = R.run(sc, torch.float64)
    n32, s32 = R.run(sc, torch.float32)
    K = sc.K
    e = R.e_ref(s32[K], s64[K])
    init = sc.init_params()
    moved = R.max_abs_diff(s64[K]["params"], init)
    print(f"[optim e_ref] {regime}: e_ref {e:.3e} = {e / sc.lr:.2e} lr, displacement {moved / sc.lr:.1f} lr, "
          f"clipped steps {R.clipped_steps(sc, n64)}/{K}")
    assert 0.0 < e < 1e-2 * sc.lr
    assert moved > 10 * sc.lr  # the parameters really travelled: e_ref is small against the path, not against nothing
    for key in ("exp_avg", "exp_avg_sq"):
        assert 0.0 < R.e_ref(s32[K], s64[K], key) < 1e-4 * R.max_abs(s64[K][key])
    # the fp32 norm of the restatement itself sits well inside the project's 1e-4
    assert max(abs(a - b) / max(b, 1e-300) for a, b in zip(n32, n64) if b > 0) < 1e-5
    # the regimes do what their names say
    c = R.clipped_steps(sc, n64)
    if regime in ("clip_all",):
        assert c == K
    if regime in ("clip_some_decay", "prescale_clip", "max_norm_switch"):
        assert 0.2 * K <= c <= 0.8 * K
    if regime in ("prescale_decay", "tiny_grads"):
        assert c == 0
    if regime == "zero_step":
        assert sum(1 for v in n64 if v == 0.0) == 3


def test_restatement_matches_the_scenario_semantics():
    """Scaling gradients by 8 and pre-scaling by 1/8 is exact in binary floating point: same float64 trajectory."""
    a = R.Scenario("ragged", "prescale_decay", 20)
    b = R.Scenario("ragged", "prescale_decay", 20)
    b.gscale, b.prescale = [1.0] * 20, [1.0] * 20
    _, sa = R.run(a, torch.float64)
    _, sb = R.run(b, torch.float64)
    for x, y in zip(sa[20]["params"], sb[20]["params"]):
        assert torch.equal(x, y)
    assert sa[20]["step"] == 20.0 and math.isclose(sa[20]["lr"], 5e-3 * 0.999977 ** 20, rel_tol=1e-14)


@pytest.mark.parametrize("norm,skip,want", [
    (float("nan"), 10.0, False),   # the reference's `norm <= skip` is False for NaN: the step is dropped
    (float("inf"), 10.0, False),
    (10.0, 10.0, True),            # equal to the threshold: steps
    (9.0, 10.0, True),
    (10.000001, 10.0, False),
    (float("nan"), None, True),    # no skip_grad_norm: the reference always steps
    (float("inf"), 0, True),       # 0 is "unset" in the reference (`not self.skip_grad_norm`)
    (1e30, None, True),
])
def test_step_skip_predicate(norm, skip, want):
    from pytorch_generative_amd import trainer

    assert bool(trainer.should_step(norm, skip)) is want
    # the same decision as the reference's expression, evaluated on a tensor as it does
    t = torch.tensor(norm)
    assert bool(not skip or t.item() <= skip) is want


def test_eager_step_uses_the_predicate():
    """Both branches of Trainer._eager_step (FlatAdam, stock optimiser) decide through should_step, not through
    `norm > skip` (which takes a NaN step)."""
    import inspect

    from pytorch_generative_amd import trainer

    src = inspect.getsource(trainer.Trainer._eager_step)
    assert src.count("should_step(") == 2 and "> self.skip_grad_norm" not in src
