"""Writes tests/golden/ref_trainer_clip/steps.pt — what the REFERENCE's own Trainer._train_one_batch
(pytorch_generative/trainer.py:173-193, on the CPU, tensorboard stubbed as in make_ckpt_golden.py) does with
`clip_grad_norm` and `skip_grad_norm` over a fixed list of batches. Build container only:

    python tests/golden/make_clip_golden.py

Three configurations — clip only, skip only, both — of the small PixelCNN of make_ckpt_golden.py. Batches: ordinary
Bernoulli images (norm below the clip threshold), "loud" ones (pixel values 0 / 3: norm above the clip threshold, below
the skip threshold), one with out-of-range targets (pixel values 0 / 60: a finite norm far above the skip threshold) and
one that contains NaN (NaN loss and norm). The clip-only configuration gets no NaN batch: the reference has nothing
that would drop it there and every parameter would turn NaN. Recorded per step: the batch, the returned metrics, whether
the optimiser stepped (Adam's step counter), the scheduler's lr, the gradients (pre-clip) and the model state afterwards.
Asserted here, so that the fixture shows every behaviour by itself: each configuration clips at least once and leaves
at least one step unclipped, skips on a finite norm and on a NaN norm where it has the feature, takes normal steps after
each skipped one, and every finite norm is at least 10 % away from each threshold it is compared with.
"""

import math
import os
import sys
import tempfile

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
OUT = os.path.join(HERE, "ref_trainer_clip")

import _ref  # noqa: E402
from make_ckpt_golden import MODEL_KW, _stub_tensorboard  # noqa: E402

LR, DECAY = 1e-3, 0.9
CLIP, SKIP = 40.0, 1000.0
CONFIGS = {"clip": dict(clip_grad_norm=CLIP), "skip": dict(skip_grad_norm=SKIP),
           "both": dict(clip_grad_norm=CLIP, skip_grad_norm=SKIP)}
KINDS = {"clip": ["plain", "loud", "plain", "wild", "plain", "loud", "plain", "plain"],
         "skip": ["plain", "loud", "wild", "plain", "nan", "plain", "loud", "plain"],
         "both": ["plain", "loud", "wild", "plain", "nan", "plain", "loud", "plain"]}


def batch(kind, i, shape=(4, 1, 8, 8)):
    g = torch.Generator().manual_seed(100 + i)
    x = torch.bernoulli(torch.full(shape, 0.3), generator=g)
    if kind == "loud":
        x = x * 3.0
    elif kind == "wild":
        x = x * 60.0
    elif kind == "nan":
        x[1, 0, 3, 4] = float("nan")
        x[2, 0, 0, 1] = float("nan")
    return x


def main():
    _stub_tensorboard()
    ref = _ref.load()
    import importlib

    import torch.nn.functional as F

    rtrainer = importlib.import_module("pytorch_generative.trainer")

    def loss_fn(x, _, preds):
        n = x.shape[0]
        return F.binary_cross_entropy_with_logits(preds.view(n, -1), x.view(n, -1), reduction="none").sum(dim=1).mean()

    out = {"model_kwargs": MODEL_KW, "lr": LR, "decay": DECAY, "configs": {}}
    for name, kw in CONFIGS.items():
        torch.manual_seed(0)
        model = ref.models.PixelCNN(**MODEL_KW)
        opt = torch.optim.Adam(model.parameters(), lr=LR)
        sched = torch.optim.lr_scheduler.MultiplicativeLR(opt, lr_lambda=lambda _: DECAY)
        log_dir = tempfile.mkdtemp()
        t = rtrainer.Trainer(model, loss_fn, opt, [], [], lr_scheduler=sched, log_dir=log_dir, n_gpus=0, **kw)
        first = next(iter(model.parameters()))
        steps, state0 = [], _ref.clone_state(model)

        # the pre-clip gradients of a step: what backward() leaves, read by a hook on the reference's own loss call
        grads = {}
        orig = t.train_one_batch

        def spy(x, y, orig=orig):
            loss = orig(x, y)
            g = torch.autograd.grad(loss, list(model.parameters()), retain_graph=True, allow_unused=True)
            grads.clear()
            grads.update({k: (None if v is None else v.detach().clone()) for (k, _), v in zip(model.named_parameters(), g)})
            return loss

        t.train_one_batch = spy
        for i, kind in enumerate(KINDS[name]):
            x = batch(kind, i)
            before = float(opt.state[first]["step"]) if opt.state else 0.0
            metrics = t._train_one_batch(x, None)
            after = float(opt.state[first]["step"]) if opt.state else 0.0
            steps.append({"kind": kind, "x": x, "metrics": metrics, "stepped": after == before + 1,
                          "adam_step": after, "lr": opt.param_groups[0]["lr"], "grads": dict(grads),
                          "state": _ref.clone_state(model)})
            print(name, i, kind, metrics, "stepped" if steps[-1]["stepped"] else "SKIPPED", opt.param_groups[0]["lr"])

        clip, skip = kw.get("clip_grad_norm"), kw.get("skip_grad_norm")
        norms = [s["metrics"]["grad_norm"] for s in steps]
        finite = [n for n in norms if math.isfinite(n)]
        for n in finite:
            for thr in (clip, skip):
                assert thr is None or abs(n - thr) >= 0.1 * thr, (name, n, thr)
        if clip:
            assert any(n > clip for n in finite) and any(n < clip for n in finite)
            assert any(s["stepped"] and s["metrics"]["grad_norm"] > clip for s in steps)
        if skip:
            assert any(math.isfinite(n) and n > skip for n in norms) and any(math.isnan(n) for n in norms)
            for i, s in enumerate(steps):
                want = not (s["metrics"]["grad_norm"] <= skip)
                assert (not s["stepped"]) == want
                if not s["stepped"]:
                    assert steps[i + 1]["stepped"], "a normal step must follow every skipped one"
                    prev = steps[i - 1]["state"]
                    # unchanged bit for bit — except the masked taps, which the forward itself zeroes
                    # (`weight.data *= mask`, nn/convolution.py:42) after the previous step moved them
                    bad = [k for k, v in s["state"].items() if not bool(((v == prev[k]) | (v == 0)).all())]
                    assert not bad, bad
        else:
            assert all(s["stepped"] for s in steps)
        assert all(bool(torch.isfinite(v).all()) for v in steps[-1]["state"].values())
        out["configs"][name] = {"kwargs": kw, "state0": state0, "steps": steps}

    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "steps.pt")
    torch.save(out, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
