"""NICE from its formulas, float64 on the CPU (the yardstick of tests/test_nice_cpu.py and tests/test_gpu_nice.py); no autograd.

A state is a dict with the model's state_dict keys: `net.{b}.net.{2 l}.weight / .bias` for layer l of block b (ReLU after every
layer but the last) and `scaling.log_scale` (1, F). Block b transforms the second half when b is even (reverse = False), the
first half when b is odd:

    forward   y_t = x_t + m_b(x_p), y_p = x_p for b = 0 .. B - 1;  z = y exp(s);  log det J = sum(s)
    inverse   y = z exp(-s);  x_t = y_t - m_b(y_p) for b = B - 1 .. 0
    loss      lp_n = -sum_j (|z| + 2 log1p(exp(-|z|)));  loss = -(mean_n lp_n + log det J)
    gradients dL/dz = tanh(z / 2) / N;  ds = sum_n dz z - 1;  dy = dz exp(s);  per block, with g the gradient of its output:
              dm = g_t, back through the layers (dW_l = d_l^T h_{l-1}, db_l = sum_n d_l, d_{l-1} = (d_l W_l) [h_{l-1} > 0]),
              gradient of its input: g_t for the transformed half, g_p + d_0 W_0 for the other."""

import torch


def n_blocks(state):
    return 1 + max(int(k.split(".")[1]) for k in state if k.startswith("net."))


def layers_of(state, b):
    """[(weight, bias), ...] of block b in float64."""
    idx = sorted({int(k.split(".")[3]) for k in state if k.startswith(f"net.{b}.net.")})
    return [(state[f"net.{b}.net.{i}.weight"].double(), state[f"net.{b}.net.{i}.bias"].double()) for i in idx]


def layer_keys(state, b):
    idx = sorted({int(k.split(".")[3]) for k in state if k.startswith(f"net.{b}.net.")})
    return [(f"net.{b}.net.{i}.weight", f"net.{b}.net.{i}.bias") for i in idx]


def _halves(f, b):
    """(pass-through slice, transformed slice) of block b."""
    first, second = slice(0, f // 2), slice(f // 2, f)
    return (second, first) if b % 2 else (first, second)


def mlp(h, layers):
    """(output, pre-activations of the hidden layers, inputs of every layer)."""
    pre, inputs = [], []
    for li, (w, b) in enumerate(layers):
        inputs.append(h)
        a = h @ w.t() + b
        if li < len(layers) - 1:
            pre.append(a)
            h = torch.relu(a)
        else:
            h = a
    return h, pre, inputs


def blocks_forward(x, state):
    """(y before the scaling, per block (pre-activations, layer inputs))."""
    y = x.double().reshape(x.shape[0], -1).clone()
    f = y.shape[1]
    tape = []
    for b in range(n_blocks(state)):
        p, t = _halves(f, b)
        m, pre, inputs = mlp(y[:, p], layers_of(state, b))
        y = y.clone()
        y[:, t] = y[:, t] + m
        tape.append((pre, inputs))
    return y, tape


def forward(x, state):
    """(z (N, F), log det J) in float64."""
    y, _ = blocks_forward(x, state)
    s = state["scaling.log_scale"].double().reshape(1, -1)
    return y * torch.exp(s), s.sum()


def inverse(z, state):
    y = z.double().reshape(z.shape[0], -1) * torch.exp(-state["scaling.log_scale"].double().reshape(1, -1))
    f = y.shape[1]
    for b in reversed(range(n_blocks(state))):
        p, t = _halves(f, b)
        m, _, _ = mlp(y[:, p], layers_of(state, b))
        y = y.clone()
        y[:, t] = y[:, t] - m
    return y


def log_prob(z):
    a = z.double().reshape(z.shape[0], -1).abs()
    return -(a + 2 * torch.log1p(torch.exp(-a))).sum(1)


def recipe_loss(z, log_det_j):
    """The recipe's dict and dL/dz."""
    z = z.double().reshape(z.shape[0], -1)
    prior = log_prob(z).mean()
    return ({"loss": -(prior + log_det_j), "prior_log_likelihood": prior, "log_det_J": log_det_j},
            torch.tanh(z / 2) / z.shape[0])


def grads_from(x, state, dz, d_log_det=0.0):
    """({key: gradient} of every parameter, gradient of x) from dz = dL/dz and d_log_det = dL/d(log det J), float64."""
    y, tape = blocks_forward(x, state)
    s = state["scaling.log_scale"].double().reshape(1, -1)
    dz = dz.double().reshape(y.shape)
    z = y * torch.exp(s)
    out = {"scaling.log_scale": ((dz * z).sum(0, keepdim=True) + d_log_det).reshape(state["scaling.log_scale"].shape)}
    g = dz * torch.exp(s)
    f = y.shape[1]
    for b in reversed(range(n_blocks(state))):
        p, t = _halves(f, b)
        pre, inputs = tape[b]
        layers, keys = layers_of(state, b), layer_keys(state, b)
        d = g[:, t]
        for li in reversed(range(len(layers))):
            out[keys[li][0]] = d.t() @ inputs[li]
            out[keys[li][1]] = d.sum(0)
            d = d @ layers[li][0]
            if li > 0:
                d = d * (pre[li - 1] > 0)
        g = g.clone()
        g[:, p] = g[:, p] + d
    return out, g


def grads(x, state):
    """The gradients of the recipe's loss, float64."""
    z, ldj = forward(x, state)
    _, dz = recipe_loss(z, ldj)
    return grads_from(x, state, dz, d_log_det=-1.0)[0]


def relu_margin(x, state):
    """min over the hidden layers of min |pre-activation| / max |pre-activation| of that layer."""
    _, tape = blocks_forward(x, state)
    return min(float(a.abs().min() / a.abs().max()) for pre, _ in tape for a in pre)


def adam_first_step(param, grad, lr=1e-3, eps=1e-8):
    """torch.optim.Adam's first step from zero moments: the bias corrections cancel the (1 - beta) factors."""
    grad = grad.double()
    return param.double() - lr * grad / (grad.abs() + eps)
