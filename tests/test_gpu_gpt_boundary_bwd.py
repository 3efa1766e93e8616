"""GPU: the backward block boundary of ImageGPT in one launch (csrc/gpt_block.hip, head_tail_bwd_kernel: the head chain of block
i+1, then the tail chain of block i on the head's dx tile while it is still in registers) against the two launches it replaces.
Kernel level through the C-ABI: d_o and gx bit for bit (the two forms run the same device functions), the 14 parameter gradients
after pg_gpt_model_reduce and d_o / gx against a float64 restatement of the two half-blocks, and run-to-run equality of the
gradients, at the tile counts where the walk changes. Then the model: the switch on and off, the pending-work check, replays of
the captured step against eager steps, and a head parameter without a sink, which keeps its boundary on two launches.

Run as a script (`python tests/test_gpu_gpt_boundary_bwd.py child`) it is the fresh process of the forced-grid case."""

import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

if __name__ == "__main__":  # the child process has no conftest.py to set the path up
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "pytorch-generative_amd"), os.path.join(_root, "tests")]

import _util

pytestmark = pytest.mark.gpu

EPS = 1e-5
TOL = 1e-4  # d_o / gx against float64, max-normalised (as test_gpu_gpt_reduce.py); parameter gradients by _util.GradReport
H_PART, T_PART = 848, 2432  # floats per partial row of the head / tail job
# (N, L). The fused launch has min(ceil(tiles / 8), 512) workgroups of four waves (grid_blocks, which = 5):
#   one_tile        one workgroup, three of its waves without a tile: they load nothing and add zeros to the row
#   crosses_images  6 tiles on 4 waves: the walk of waves 0 and 1 wraps from image 0 into image 1
#   tiles_differ    245 tiles on 31 workgroups = 124 waves: 121 waves walk two tiles, 3 walk one; every last iteration re-reads
#                   its own tile
SHAPES = {"one_tile": (1, 16), "crosses_images": (2, 48), "tiles_differ": (5, 784)}
HEAD = ("ln1_w", "ln1_b", "wq", "bq", "wkv", "bkv")
TAIL = ("wp", "bp", "ln2_w", "ln2_b", "w1", "b1", "w2", "b2")
REDUCE = HEAD + ("w1", "b1", "w2", "b2", "wp", "bp", "ln2_w", "ln2_b")  # the 14 destinations of pg_gpt_model_reduce per block
# The forced-grid case: the child asks for one workgroup per kernel. Only a library built with the A/B switches live reads
# PG_BLOCK_GRID (csrc/common.h, PG_AB_ENV); there 14 tiles on 4 waves give every wave 3 or 4 iterations. The production library
# ignores it, and the child then takes a shape at which the production grid rule itself gives every wave 3 iterations (6272
# tiles on 512 workgroups = 2048 waves, the first 128 a fourth).
FORCED_GRID = "2048,1,2048,1,1536,1"
FORCED_SHAPE, THREE_ITERATION_SHAPE = (2, 112), (128, 784)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _params():
    """ln1 / q / kv of block i+1 and proj / ln2 / fc1 / fc2 of block i"""
    return {"ln1_w": 1 + _rand(16, seed=20, scale=.1), "ln1_b": _rand(16, seed=21, scale=.1),
            "wq": _rand(16, 16, seed=22, scale=.2), "bq": _rand(16, seed=23),
            "wkv": _rand(32, 16, seed=24, scale=.2), "bkv": _rand(32, seed=25),
            "wp": _rand(16, 16, seed=10, scale=.2), "bp": _rand(16, seed=11),
            "ln2_w": 1 + _rand(16, seed=12, scale=.1), "ln2_b": _rand(16, seed=13, scale=.1),
            "w1": _rand(64, 16, seed=14, scale=.2), "b1": _rand(64, seed=15),
            "w2": _rand(16, 64, seed=16, scale=.1), "b2": _rand(16, seed=17)}


def _inputs(n, L):
    """x1, gx1, dqkv: input, residual gradient and d qkv of block i+1's head; x0, o: the inputs of block i's tail"""
    return {"x1": _rand(n, 16, L, seed=1), "gx1": _rand(n, 16, L, seed=4), "dqkv": _rand(n, 48, L, seed=3),
            "x0": _rand(n, 16, L, seed=6), "o": _rand(n, 16, L, seed=2)}


def _reference(P, t):
    """float64 on the CPU, from the formulas at the top of gpt_block.hip. Head of block i+1: qkv = [Wq; Wkv] LN1(x1) + b with the
    alias of x1 receiving gx1; its dx is D = d x_new of block i's tail: x_new = x0 + x_mid + W2 gelu(W1 LN2(x_mid) + b1) + b2,
    x_mid = x0 + Wp o + bp. Returns d_o, gx (of x0) and the 14 parameter gradients."""
    P = {k: v.double().requires_grad_() for k, v in P.items()}
    x1, x0, o = (t[k].double().requires_grad_() for k in ("x1", "x0", "o"))
    ln = lambda v, w, b: F.layer_norm(v.transpose(1, 2), (16,), w, b, EPS).transpose(1, 2)  # noqa: E731
    conv = lambda v, w, b: torch.einsum("oc,ncl->nol", w, v) + b[None, :, None]  # noqa: E731
    qkv = conv(ln(x1, P["ln1_w"], P["ln1_b"]), torch.cat([P["wq"], P["wkv"]]), torch.cat([P["bq"], P["bkv"]]))
    ((qkv * t["dqkv"].double()).sum() + (x1 * t["gx1"].double()).sum()).backward()
    xm = x0 + conv(o, P["wp"], P["bp"])
    xnew = x0 + xm + conv(F.gelu(conv(ln(xm, P["ln2_w"], P["ln2_b"]), P["w1"], P["b1"])), P["w2"], P["b2"])
    (xnew * x1.grad).sum().backward()
    return {"d_o": o.grad, "gx": x0.grad, **{k: p.grad for k, p in P.items()}}


@pytest.fixture(scope="module")
def cases():
    """Per shape: parameters, inputs and the float64 reference, computed once and left unchanged."""
    P = _params()
    out = {}
    for name, (n, L) in SHAPES.items():
        t = _inputs(n, L)
        out[name] = (P, t, _reference(P, t))
    return out


def _ptrs(ts):
    return [t.data_ptr() for t in ts]


def _run(lib, dev, P, t, n, L, fused):
    """Both half-blocks on the device, fused (one launch) or as pg_gpt_block_head_bwd_partial followed by
    pg_gpt_block_tail_bwd_partial on the dx it wrote; then ONE pg_gpt_model_reduce over the two workspaces. Outputs and workspaces
    start as NaN, the gradients at zero. Returns (d_o, gx), the 14 gradients and the two workspaces."""
    st = torch.cuda.current_stream().cuda_stream
    hn, tn = lib.pg_gpt_block_head_bwd_workspace_floats(n, L), lib.pg_gpt_block_tail_bwd_workspace_floats(n, L)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)  # noqa: E731
    d_o, gx, dx, hws, tws = nan(n, 16, L), nan(n, 16, L), nan(n, 16, L), nan(hn), nan(tn)
    g = {k: torch.zeros_like(P[k]) for k in REDUCE}
    head_in = _ptrs([t["x1"], P["ln1_w"], P["ln1_b"], P["wq"], P["wkv"], t["dqkv"], t["gx1"]])
    tail_in = _ptrs([t["o"], t["x0"]] + [P[k] for k in TAIL[:-1]])
    if fused:
        assert lib.pg_gpt_block_head_tail_bwd_partial(*head_in, *tail_in, d_o.data_ptr(), gx.data_ptr(), n, 16, 64, L, EPS,
                                                      hws.data_ptr(), hn, tws.data_ptr(), tn, st) == 0
    else:
        assert lib.pg_gpt_block_head_bwd_partial(*head_in, dx.data_ptr(), n, 16, L, EPS, hws.data_ptr(), hn, st) == 0
        assert lib.pg_gpt_block_tail_bwd_partial(*tail_in, dx.data_ptr(), d_o.data_ptr(), gx.data_ptr(), n, 16, 64, L, EPS,
                                                 tws.data_ptr(), tn, st) == 0
    one = lambda p: (ctypes.c_void_p * 1)(p)  # noqa: E731
    assert lib.pg_gpt_model_reduce(1, one(hws.data_ptr()), one(tws.data_ptr()),
                                   (ctypes.c_void_p * 14)(*[g[k].data_ptr() for k in REDUCE]), n, 16, L,
                                   0, 0, 0, None, 0, 0, 0, 0, 0, None, st) == 0
    torch.cuda.synchronize()
    if fused:
        assert bool(torch.isnan(dx).all()), "the fused launch wrote a dx"
    return (d_o, gx), g, (hws, tws)


def _check_case(lib, dev, P, t, want, n, L, what):
    P, t = {k: v.to(dev) for k, v in P.items()}, {k: v.to(dev) for k, v in t.items()}
    (d_o_u, gx_u), _, ws_u = _run(lib, dev, P, t, n, L, fused=False)
    (d_o, gx), g, ws = _run(lib, dev, P, t, n, L, fused=True)
    assert bool(torch.isfinite(d_o_u).all()) and bool(torch.isfinite(gx_u).all())
    assert torch.equal(d_o, d_o_u), f"{what}: d_o of the fused launch differs from the two launches'"
    assert torch.equal(gx, gx_u), f"{what}: gx of the fused launch differs from the two launches'"
    assert bool(torch.isfinite(ws[0]).all()) and bool(torch.isfinite(ws[1]).all()), f"{what}: a partial row was left unwritten"
    _util.assert_close(d_o, want["d_o"], TOL, f"{what}: d_o")
    _util.assert_close(gx, want["gx"], TOL, f"{what}: gx")
    rep = _util.GradReport(f"gpt_boundary_bwd[{what}]")
    for k in REDUCE:
        rep.add(k, g[k], want[k])
    assert len(rep.rows) == 14
    rep.finish()
    _, g2, _ = _run(lib, dev, P, t, n, L, fused=True)
    for k in REDUCE:
        assert torch.equal(g2[k], g[k]), f"{what}: gradient of {k} differs between two runs"
    return ws, ws_u


@pytest.mark.parametrize("case", list(SHAPES))
def test_fused_boundary_backward_against_two_launches_and_float64(dev, lib, cases, case):
    n, L = SHAPES[case]
    P, t, want = cases[case]
    ws, ws_u = _check_case(lib, dev, P, t, want, n, L, case)
    if case == "one_tile":
        # one tile: the row is that tile's sums plus what the three waves without a tile add, which must be nothing
        assert ws[0].numel() == H_PART and ws[1].numel() == T_PART
        assert torch.equal(ws[0], ws_u[0]) and torch.equal(ws[1], ws_u[1]), "partial rows of one tile differ from the two launches'"


def test_forced_small_grid_in_a_fresh_process():
    """At least three iterations per wave, in a child process because the library reads PG_BLOCK_GRID once (see FORCED_GRID)."""
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=dict(os.environ, PG_BLOCK_GRID=FORCED_GRID),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:]
    assert "[child] ok" in p.stdout, p.stdout[-4000:]


def _child():
    from pytorch_generative_amd import _lib

    lib, dev = _lib.load(), torch.device("cuda:0")
    forced = lib.pg_gpt_block_head_bwd_workspace_floats(*FORCED_SHAPE) == H_PART  # 14 tiles: two rows unless the cap of 1 is live
    n, L = FORCED_SHAPE if forced else THREE_ITERATION_SHAPE
    P, t = _params(), _inputs(n, L)
    _check_case(lib, dev, P, t, _reference(P, t), n, L, f"forced grid ({'PG_BLOCK_GRID' if forced else 'by shape'})")
    print(f"[child] ok: N={n} L={L} forced={forced}")


# ------------------------------------------------------------------------------------------------ model level
def _model(dev):
    import pytorch_generative_amd as pg

    torch.manual_seed(0)
    m = pg.models.ImageGPT(1, 1, in_size=8, n_transformer_blocks=3, n_attention_heads=4, n_embedding_channels=16)
    with torch.no_grad():
        m._pos.normal_(0, 0.1)
    return m.to(dev)


def _batches(dev, k):
    g = torch.Generator().manual_seed(11)
    return [torch.bernoulli(torch.full((4, 1, 8, 8), 0.1307), generator=g).to(dev) for _ in range(k)]


BWD_LAUNCHES = ("pg_gpt_block_head_tail_bwd_partial", "pg_gpt_block_head_bwd_partial", "pg_gpt_block_tail_bwd_partial",
                "pg_gpt_block_head_bwd", "pg_gpt_block_tail_bwd")


def _count(monkeypatch, lib, calls):
    for name in BWD_LAUNCHES:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _n=name, _r=real: (calls.append(_n), _r(*a))[1], raising=False)


def _one_step(dev, lib, monkeypatch, on, x, without_sink=None):
    """One FlatAdam step of the 3-block model with the switch set. without_sink: the name of a parameter left out of the optimizer
    (it keeps requires_grad and receives a plain .grad). Returns the loss, the logits, the gradients by name, the flat gradient and
    the backward launches by name."""
    from pytorch_generative_amd import ops, optim

    calls = []
    _count(monkeypatch, lib, calls)
    monkeypatch.setattr(ops.gpt_block, "FUSE_BOUNDARY_BWD", on)
    m = _model(dev)
    opt = optim.FlatAdam([p for k, p in m.named_parameters() if k != without_sink], lr=1e-3)
    opt.zero_grad()
    logits = m(x)
    loss = ops.bce_with_logits_sum_mean(logits, x)
    loss.backward()
    torch.cuda.synchronize()
    ops.assert_no_pending_block_reductions()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    flat = opt.flat_grad.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    return float(loss), logits.detach().clone(), grads, flat, {k: calls.count(k) for k in set(calls)}


def test_model_step_with_the_switch_on_and_off(dev, lib, monkeypatch):
    """3 blocks = 2 boundaries: with the switch on both run fused, block 0's head and block 2's tail keep their own launches; off,
    three of each. Same loss bits (the forward does not depend on the switch), flat gradients within the gradient gate of each
    other and of the CPU oracle, nothing left pending."""
    from oracle import models as omodels
    from oracle import train as otrain
    from pytorch_generative_amd import ops

    x = _batches(dev, 1)[0]
    ref = _model(torch.device("cpu"))
    state = {k: v.detach().clone() for k, v in ref.state_dict().items()}
    _, _, o_grads = otrain.loss_and_grads(omodels.image_gpt, state, x.cpu(), n_heads=4)
    was = ops.set_deterministic(True)
    try:
        on = _one_step(dev, lib, monkeypatch, True, x)
        off = _one_step(dev, lib, monkeypatch, False, x)
    finally:
        ops.set_deterministic(was)
    assert on[4] == {"pg_gpt_block_head_tail_bwd_partial": 2, "pg_gpt_block_head_bwd_partial": 1, "pg_gpt_block_tail_bwd_partial": 1}, on[4]
    assert off[4] == {"pg_gpt_block_head_bwd_partial": 3, "pg_gpt_block_tail_bwd_partial": 3}, off[4]
    assert torch.equal(on[1], off[1]), "logits differ"
    assert torch.tensor(on[0]).view(torch.int32).item() == torch.tensor(off[0]).view(torch.int32).item(), "loss bits differ"
    rep = _util.GradReport("gpt_boundary_bwd[model, on vs off]")
    rep.add("flat_grad", on[3], off[3])
    rep.finish()
    for name, got in (("on", on), ("off", off)):
        rep = _util.GradReport(f"gpt_boundary_bwd[model, {name} vs oracle]")
        for k, g in got[2].items():
            rep.add(k, g, o_grads[k])
        assert len(rep.rows) == 3 + 3 * 14 + 4
        rep.finish()


def test_head_parameter_without_a_sink_keeps_two_launches(dev, lib, monkeypatch):
    """Block 1's LN1 weight outside the optimizer: its head reduces its own rows and does not defer, so the boundary 0|1 runs as
    two launches and only 1|2 fused; the gradients match those with the switch off."""
    from pytorch_generative_amd import ops

    x = _batches(dev, 1)[0]
    name = "_transformer.1._ln1.weight"
    was = ops.set_deterministic(True)
    try:
        on = _one_step(dev, lib, monkeypatch, True, x, without_sink=name)
        off = _one_step(dev, lib, monkeypatch, False, x, without_sink=name)
    finally:
        ops.set_deterministic(was)
    assert on[4] == {"pg_gpt_block_head_tail_bwd_partial": 1, "pg_gpt_block_head_bwd_partial": 2, "pg_gpt_block_tail_bwd_partial": 2}, on[4]
    assert off[4] == {"pg_gpt_block_head_bwd_partial": 3, "pg_gpt_block_tail_bwd_partial": 3}, off[4]
    assert on[0] == off[0] and name in on[2]
    rep = _util.GradReport("gpt_boundary_bwd[model, head parameter without a sink]")
    for k, g in on[2].items():
        rep.add(k, g, off[2][k])
    assert len(rep.rows) == 3 + 3 * 14 + 4
    rep.finish()


def test_graph_replays_of_the_fused_step_equal_eager_steps(dev):
    """Three replays of the captured step equal three eager steps bit for bit under ops.set_deterministic(True); the fused
    backward boundary is selected whatever the switch's default."""
    from pytorch_generative_amd import graph, ops, optim

    xs = _batches(dev, 3)
    loss_fn = lambda x, preds: ops.bce_with_logits_sum_mean(preds, x)  # noqa: E731
    was, sw = ops.set_deterministic(True), ops.gpt_block.FUSE_BOUNDARY_BWD
    ops.gpt_block.FUSE_BOUNDARY_BWD = True
    try:
        m1, m2 = _model(dev), _model(dev)
        o1, o2 = optim.FlatAdam(m1.parameters(), lr=1e-3), optim.FlatAdam(m2.parameters(), lr=1e-3)
        for x in xs:
            o1.zero_grad()
            loss_fn(x, m1(x)).backward()
            o1.step()
        step = graph.GraphedTrainStep(m2, o2, loss_fn, xs[0], preserve_state=True)
        for x in xs:
            step(x)
        torch.cuda.synchronize()
        assert torch.equal(o1.flat_param, o2.flat_param), "graph replays differ from eager steps"
        assert torch.equal(o1.exp_avg, o2.exp_avg) and torch.equal(o1.exp_avg_sq, o2.exp_avg_sq)
    finally:
        ops.gpt_block.FUSE_BOUNDARY_BWD = sw
        ops.set_deterministic(was)


if __name__ == "__main__":
    assert sys.argv[1:] == ["child"], sys.argv
    _child()
