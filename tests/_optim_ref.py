"""The optimiser half of the step, restated on the CPU for the FlatAdam tests (GPU and CPU tier).

One step of the reference (trainer.py:183-191, with the 1/world of the data-parallel path in front):

    g *= prescale; clip_grad_norm_(params, max_norm or 1e50); Adam.step(); lr *= decay

`run()` plays a `Scenario` through exactly that — `torch.nn.utils.clip_grad_norm_` and `torch.optim.Adam`
on clones of the parameters, nothing re-derived by hand — in float64 (the truth) or in float32 (the
reference's own arithmetic: its distance to float64, `e_ref`, is the yardstick the kernel is held to).
The gradient stream does not depend on the parameters, so nothing amplifies a rounding difference.
"""

import math

import torch

BETAS, EPS = (0.9, 0.999), 1e-8
TWO_M23 = 2.0 ** -23

# name -> [(shape, index of the parameter it follows or None)]
LAYOUTS = {
    "n1": [((1,), None)],
    "n3": [((3,), None)],
    "n4": [((4,), None)],
    "n5": [((5,), None)],
    "ragged": [((7,), None), ((3, 5), None), ((1,), None), ((64, 33), None)],
    # q / kv style pair: the follower sits directly behind its leader (8 elements, no padding), then a padded tail
    "follows": [((2, 4), None), ((3, 3), 0), ((5,), None)],
    "n4099": [((4099,), None)],
    # above pg_adam_step's cap (2048 blocks x 256 elements) and below pg_sumsq's (1024 blocks x 256 float4)
    "mid": [((700001,), None)],
    # above both caps, length not a multiple of 4 before padding
    "big": [((3000001,), None)],
}
SMALL = ("n1", "n3", "n4", "n5", "ragged", "follows")
REGIMES = ("clip_all", "clip_some_decay", "prescale_decay", "tiny_grads", "prescale_clip", "zero_step", "max_norm_switch")  # + "zeros_only": its own exactness test


def numel(layout):
    return sum(math.prod(s) for s, _ in LAYOUTS[layout])


class Scenario:
    """A layout, K steps and per step: the gradient's scale, the pre-scale, max_norm (None = unset)."""

    def __init__(self, layout, regime, K, seed=0):
        self.layout, self.regime, self.K, self.seed = layout, regime, K, seed
        self.shapes = [s for s, _ in LAYOUTS[layout]]
        self.follows = [f for _, f in LAYOUTS[layout]]
        root_n = math.sqrt(numel(layout))
        self.lr, self.decay = 1e-3, 1.0
        self.gscale, self.prescale, self.max_norm = [1.0] * K, [1.0] * K, [None] * K
        # every gradient element is z + 0.25 sign(z), z unit normal: |g| >= 0.25 scale, so
        # 0.25 scale sqrt(n) <= norm, and a max_norm below that clips on EVERY step whatever n is
        if regime == "clip_all":
            self.max_norm = [0.05 * root_n] * K
        elif regime == "clip_some_decay":
            self.gscale = [8.0 if k % 3 == 0 else 0.125 for k in range(K)]
            self.max_norm = [0.6 * root_n] * K
            self.decay = 0.99
        elif regime == "prescale_decay":  # the ImageGPT recipe's lr and decay, the all-reduce's 1/world
            self.gscale, self.prescale = [8.0] * K, [0.125] * K
            self.lr, self.decay = 5e-3, 0.999977
        elif regime == "tiny_grads":  # sqrt(v) ~ 1e-6: eps = 1e-8 is ~1 % of the denominator
            self.gscale = [1e-6] * K
            self.max_norm = [1.0] * K
        elif regime == "prescale_clip":  # pre enters twice: norm = sqrt(sumsq) pre, g *= coef pre
            self.gscale = [8.0 if k % 3 == 0 else 0.125 for k in range(K)]
            self.prescale = [(0.25, 0.5, 1.0 / 3.0)[(k // 2) % 3] for k in range(K)]
            self.max_norm = [0.2 * root_n] * K
            self.decay = 0.995
        elif regime == "zero_step":
            self.max_norm = [0.05 * root_n] * K
            for k in (K // 2, K // 2 + 1, K - 2):
                self.gscale[k] = 0.0
        elif regime == "max_norm_switch":  # None -> finite -> None
            self.max_norm = [None if (k < K // 3 or k >= 2 * K // 3) else 0.05 * root_n for k in range(K)]
        elif regime == "zeros_only":
            self.gscale = [0.0] * K
            self.max_norm = [1.0] * K
        else:
            raise KeyError(regime)
        self._grads = {}

    def checkpoints(self):
        return sorted({k for k in (1, 2, 10, self.K // 2, self.K) if 1 <= k <= self.K})

    def init_params(self):
        g = torch.Generator().manual_seed(1000 + self.seed)
        return [torch.randn(s, generator=g) for s in self.shapes]

    def grads(self, k):
        """fp32 gradients of step k (0-based), BEFORE the pre-scale; cached (three consumers)."""
        if k not in self._grads:
            g = torch.Generator().manual_seed(7919 * (self.seed + 1) + k)
            out = []
            for s in self.shapes:
                z = torch.randn(s, generator=g)
                out.append((z + 0.25 * torch.sign(z)) * self.gscale[k])
            self._grads[k] = out
        return self._grads[k]


def run(sc, dtype):
    """Plays `sc` through clip_grad_norm_ + torch.optim.Adam in `dtype`. Returns (norms, snaps): the pre-clip
    norm of every step as a Python float, and at each of sc.checkpoints() a dict with the parameters, both
    moments, the lr the NEXT step uses and the step count."""
    params = [torch.nn.Parameter(p.to(dtype).clone()) for p in sc.init_params()]
    opt = torch.optim.Adam(params, lr=sc.lr, betas=BETAS, eps=EPS)
    lr, norms, snaps, marks = sc.lr, [], {}, set(sc.checkpoints())
    for k in range(sc.K):
        for p, g in zip(params, sc.grads(k)):
            p.grad = g.to(dtype) * sc.prescale[k]
        norm = torch.nn.utils.clip_grad_norm_(params, 1e50 if sc.max_norm[k] is None else sc.max_norm[k])
        norms.append(float(norm))
        opt.step()
        lr *= sc.decay
        opt.param_groups[0]["lr"] = lr
        if k + 1 in marks:
            snaps[k + 1] = {
                "params": [p.detach().clone() for p in params],
                "exp_avg": [opt.state[p]["exp_avg"].clone() for p in params],
                "exp_avg_sq": [opt.state[p]["exp_avg_sq"].clone() for p in params],
                "lr": lr, "step": float(opt.state[params[0]]["step"]),
            }
    return norms, snaps


def max_abs_diff(a, b):
    return max(float((x.double() - y.double()).abs().max()) for x, y in zip(a, b))


def max_abs(a):
    return max(float(x.double().abs().max()) for x in a)


def e_ref(snap32, snap64, key="params"):
    """max |fp32 restatement - float64 restatement| over a checkpoint's tensors: the reference's own error."""
    return max_abs_diff(snap32[key], snap64[key])


def bound(snap32, snap64, key="params"):
    """What the kernel may differ from float64 by: 4 e_ref + 1e-7 max|x|. The 4 covers another summation order
    in the norm and powf against Python's **; it is not a measured-and-padded figure."""
    return 4.0 * e_ref(snap32, snap64, key) + 1e-7 * max_abs(snap64[key])


def clipped_steps(sc, norms64):
    return sum(1 for k in range(sc.K) if sc.max_norm[k] is not None and norms64[k] > sc.max_norm[k])
