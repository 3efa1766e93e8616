"""GPU: the one segmented-reduce kernel of csrc/gpt_block.hip (seg_reduce_kernel) and the one path to it. The partial rows of a
block's head and tail backward kernels become gradients on three routes — at once after each kernel, parked and added by
pg_gpt_model_reduce for one block, parked and added together with another block's — and every route runs the same kernel over the
same rows in the same order, so the gradients must be the same bits. Kernel level through the C-ABI at the row counts where the
kernel's row loop changes regime, then the model: the routes that ImageGPT selects from what it can observe (a stem that flushes,
a first block that flushes, blocks that reduce their own rows, kernels that reduce their own rows) and a model of more than eight
blocks, whose rows need a second launch."""

import ctypes

import pytest
import torch
import torch.nn.functional as F

import _util

pytestmark = pytest.mark.gpu

EPS = 1e-5
TOL = 1e-4  # as test_gpu_gpt_block_pipeline.py: activations gradients max-normalised, parameter gradients by _util.GradReport
H_PART, T_PART = 848, 2432  # floats per partial row of the head / tail backward kernel
# partial rows -> (N, L). The backward kernels run ceil(N * L / 16 / 8) workgroups (below their caps) and leave one row each; the
# reduce kernel's 32 row groups walk rows rg, rg + 32 in pairs (stride 64) and then a remainder row: 1 row = remainder only;
# 33 = one paired iteration for row group 0, remainder for the others; 70 = a paired iteration for every group and a remainder
# for groups 0..5 only
SHAPES = {1: (1, 128), 33: (3, 1408), 70: (5, 1792)}
HEAD = ("ln1_w", "ln1_b", "wq", "bq", "wkv", "bkv")                      # gradient order of pg_gpt_block_head_bwd
TAIL = ("wp", "bp", "ln2_w", "ln2_b", "w1", "b1", "w2", "b2")            # gradient order of pg_gpt_block_tail_bwd
REDUCE = HEAD + ("w1", "b1", "w2", "b2", "wp", "bp", "ln2_w", "ln2_b")   # the 14 destinations of pg_gpt_model_reduce per block
REMOVED = ("pg_gpt_block_head_bwd_with_tail", "pg_gpt_blocks_reduce")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _block_params(s):
    return {"ln1_w": 1 + _rand(16, seed=s + 20, scale=.1), "ln1_b": _rand(16, seed=s + 21, scale=.1),
            "wq": _rand(16, 16, seed=s + 22, scale=.2), "bq": _rand(16, seed=s + 23),
            "wkv": _rand(32, 16, seed=s + 24, scale=.2), "bkv": _rand(32, seed=s + 25),
            "wp": _rand(16, 16, seed=s + 10, scale=.2), "bp": _rand(16, seed=s + 11),
            "ln2_w": 1 + _rand(16, seed=s + 12, scale=.1), "ln2_b": _rand(16, seed=s + 13, scale=.1),
            "w1": _rand(64, 16, seed=s + 14, scale=.2), "b1": _rand(64, seed=s + 15),
            "w2": _rand(16, 64, seed=s + 16, scale=.1), "b2": _rand(16, seed=s + 17)}


def _block_inputs(n, L, s):
    return {"x": _rand(n, 16, L, seed=s + 1), "o": _rand(n, 16, L, seed=s + 2), "dqkv": _rand(n, 48, L, seed=s + 3),
            "gx": _rand(n, 16, L, seed=s + 4), "d": _rand(n, 16, L, seed=s + 5)}


def _reference(P, t):
    """float64 restatement on the CPU: head qkv = [Wq; Wkv] LN1(x) + b with the alias x (gradient gx); tail x_new = x + x_mid +
    mlp(LN2(x_mid)), x_mid = x + Wp o + bp. Returns dx, d_o, gx (of the tail's x) and the 14 parameter gradients."""
    P = {k: v.double().requires_grad_() for k, v in P.items()}
    x, o, xt = (t[k].double().requires_grad_() for k in ("x", "o", "x"))
    ln = lambda v, w, b: F.layer_norm(v.transpose(1, 2), (16,), w, b, EPS).transpose(1, 2)  # noqa: E731
    conv = lambda v, w, b: torch.einsum("oc,ncl->nol", w, v) + b[None, :, None]  # noqa: E731
    qkv = conv(ln(x, P["ln1_w"], P["ln1_b"]), torch.cat([P["wq"], P["wkv"]]), torch.cat([P["bq"], P["bkv"]]))
    xm = xt + conv(o, P["wp"], P["bp"])
    xnew = xt + xm + conv(F.gelu(conv(ln(xm, P["ln2_w"], P["ln2_b"]), P["w1"], P["b1"])), P["w2"], P["b2"])
    ((qkv * t["dqkv"].double()).sum() + (x * t["gx"].double()).sum() + (xnew * t["d"].double()).sum()).backward()
    return {"dx": x.grad, "d_o": o.grad, "gx": xt.grad, **{k: p.grad for k, p in P.items()}}


@pytest.fixture(scope="module")
def cases():
    """Per row count two independent blocks (parameters, inputs, float64 reference), computed once and left unchanged."""
    out = {}
    for rows, (n, L) in SHAPES.items():
        out[rows] = []
        for s in (0, 100):
            P, t = _block_params(s), _block_inputs(n, L, s)
            out[rows].append((P, t, _reference(P, t)))
    return out


def _ptrs(ts):
    return [t.data_ptr() for t in ts]


def _array(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _run(lib, dev, blocks, n, L, parked):
    """The backward kernels of every block in `blocks` = [(parameters, inputs)], both on the device. parked=False: each kernel
    reduces its own rows (pg_gpt_block_tail_bwd, pg_gpt_block_head_bwd); parked=True: the _partial entry points and ONE
    pg_gpt_model_reduce over all the blocks, without ends. Every gradient destination starts at 0.25 (the reductions add),
    dx / d_o / gx at NaN. Returns [(gradients, outputs)] per block."""
    st = torch.cuda.current_stream().cuda_stream
    hn, tn = lib.pg_gpt_block_head_bwd_workspace_floats(n, L), lib.pg_gpt_block_tail_bwd_workspace_floats(n, L)
    res, left = [], []
    for P, t in blocks:
        g = {k: torch.full_like(P[k], 0.25) for k in REDUCE}
        out = {k: torch.full((n, 16, L), float("nan"), device=dev) for k in ("dx", "d_o", "gx")}
        hws, tws = torch.empty(hn, device=dev), torch.empty(tn, device=dev)
        tail_in = _ptrs([t["o"], t["x"]] + [P[k] for k in TAIL[:-1]] + [t["d"], out["d_o"], out["gx"]])
        head_in = _ptrs([t["x"], P["ln1_w"], P["ln1_b"], P["wq"], P["wkv"], t["dqkv"], t["gx"], out["dx"]])
        if parked:
            assert lib.pg_gpt_block_tail_bwd_partial(*tail_in, n, 16, 64, L, EPS, tws.data_ptr(), tn, st) == 0
            assert lib.pg_gpt_block_head_bwd_partial(*head_in, n, 16, L, EPS, hws.data_ptr(), hn, st) == 0
            left.append((hws, tws, g))
        else:
            assert lib.pg_gpt_block_tail_bwd(*tail_in, *_ptrs(g[k] for k in TAIL), n, 16, 64, L, EPS, tws.data_ptr(), tn, st) == 0
            assert lib.pg_gpt_block_head_bwd(*head_in, *_ptrs(g[k] for k in HEAD), n, 16, L, EPS, hws.data_ptr(), hn, st) == 0
        res.append((g, out))
    if left:
        assert lib.pg_gpt_model_reduce(len(left), _array(_ptrs(h for h, _, _ in left)), _array(_ptrs(w for _, w, _ in left)),
                                       _array([g[k].data_ptr() for _, _, g in left for k in REDUCE]), n, 16, L,
                                       0, 0, 0, None, 0, 0, 0, 0, 0, None, st) == 0
    torch.cuda.synchronize()
    return res


def _assert_same_bits(got, want, what):
    for part_g, part_w in zip(got, want):
        assert part_g.keys() == part_w.keys()
        for k in part_w:
            assert torch.equal(part_g[k], part_w[k]), f"{what}: {k} differs"


@pytest.mark.parametrize("rows", list(SHAPES))
def test_reduce_routes_of_the_c_abi_agree_bitwise(dev, lib, cases, rows):
    n, L = SHAPES[rows]
    assert lib.pg_gpt_block_head_bwd_workspace_floats(n, L) == rows * H_PART
    assert lib.pg_gpt_block_tail_bwd_workspace_floats(n, L) == rows * T_PART
    blocks = [({k: v.to(dev) for k, v in P.items()}, {k: v.to(dev) for k, v in t.items()}) for P, t, _ in cases[rows]]
    at_once = [_run(lib, dev, [b], n, L, parked=False)[0] for b in blocks]  # (a), each block on its own
    # (a) is right, so the comparisons below are not between two copies of garbage
    for i, ((g, out), (_, _, want)) in enumerate(zip(at_once, cases[rows])):
        for k in out:
            _util.assert_close(out[k], want[k], TOL, f"{rows} rows, block {i}: {k}")
        rep = _util.GradReport(f"gpt_reduce[{rows} rows, block {i}]")
        for k in REDUCE:
            rep.add(k, g[k].double() - 0.25, want[k])
        assert len(rep.rows) == 14
        rep.finish()
    for i, b in enumerate(blocks):  # (b) parked, then one reduce of one block
        _assert_same_bits(_run(lib, dev, [b], n, L, parked=True)[0], at_once[i], f"{rows} rows: one parked block ({i})")
    both = _run(lib, dev, blocks, n, L, parked=True)  # (c) two blocks parked, one reduce of two
    for i in range(2):
        _assert_same_bits(both[i], at_once[i], f"{rows} rows: block {i} of two parked blocks")


# ------------------------------------------------------------------------------------------------ model level
def _model(dev, n_blocks, frozen_stem=False):
    import pytorch_generative_amd as pg

    torch.manual_seed(0)
    m = pg.models.ImageGPT(1, 1, in_size=8, n_transformer_blocks=n_blocks, n_attention_heads=4, n_embedding_channels=16)
    with torch.no_grad():
        m._pos.normal_(0, 0.1)
    if frozen_stem:
        for p in (m._pos, m._input.weight, m._input.bias):
            p.requires_grad_(False)
    return m.to(dev)


def _batch(dev, n=2):
    return torch.bernoulli(torch.full((n, 1, 8, 8), 0.1307), generator=torch.Generator().manual_seed(11)).to(dev)


def _record_reduces(monkeypatch, lib, calls):
    """calls collects n_blocks of every pg_gpt_model_reduce call"""
    real = lib.pg_gpt_model_reduce
    monkeypatch.setattr(lib, "pg_gpt_model_reduce", lambda *a: (calls.append(a[0]), real(*a))[1], raising=False)


def _backward(m, x, sinks, forward=None):
    """One backward pass; sinks=True: under FlatAdam over the model's trainable parameters. Returns the gradients by name."""
    from pytorch_generative_amd import ops, optim

    if sinks:
        optim.FlatAdam(m.parameters(), lr=1e-3).zero_grad()
    ops.bce_with_logits_sum_mean((forward or m)(x), x).backward()
    torch.cuda.synchronize()
    ops.assert_no_pending_block_reductions()
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def _first_block_flushes(m):
    """ImageGPT.forward as it runs the blocks when nothing in front of them flushes (a stem off the fused shape): one chain for all
    blocks, flushed by the first block's backward, the output head outside it. The stem's output is a leaf here."""
    from pytorch_generative_amd import ops

    def forward(img):
        with torch.no_grad():
            x = m._input(img, pos=m._pos)
        x.requires_grad_(True)
        x = ops.gpt_blocks(x, list(m._transformer), ops.new_block_chain(), flush=True)
        return m._out(x, pre_ln=m._ln)

    return forward


def test_model_routes_agree_bitwise_and_launch_as_counted(dev, lib, monkeypatch):
    """A 2-block ImageGPT, one backward pass on every route; n_blocks of the pg_gpt_model_reduce calls in backward order:
      chain      everything under FlatAdam: the stem flushes both blocks and both ends                       [2]
      own_rows   FlatAdam over everything but a frozen stem: the output head, then each block for itself     [0, 1, 1]
      first      the same model with the blocks run as ImageGPT.forward runs them behind a stem that does
                 not flush: the output head, then the first block flushes both                              [0, 2]
      no_sinks   plain .grad: every block kernel reduces its own rows; the output head, then the stem        [0, 0]
    ImageGPT.forward declines the chain when the first block's input needs no gradient, so a frozen stem selects own_rows and
    not first; first is therefore driven through ops.gpt_blocks."""
    from pytorch_generative_amd import ops

    for name in REMOVED:
        assert not hasattr(lib, name), f"{name} is still exported"
    calls = []
    _record_reduces(monkeypatch, lib, calls)
    x = _batch(dev)
    want_calls = {"chain": [2], "own_rows": [0, 1, 1], "first": [0, 2], "no_sinks": [0, 0]}
    was = ops.set_deterministic(True)
    try:
        got = {}
        for route in want_calls:
            del calls[:]
            m = _model(dev, 2, frozen_stem=route in ("own_rows", "first"))
            got[route] = _backward(m, x, sinks=route != "no_sinks", forward=_first_block_flushes(m) if route == "first" else None)
            assert calls == want_calls[route], f"{route}: pg_gpt_model_reduce calls {calls}"
    finally:
        ops.set_deterministic(was)
    stem = {"_pos", "_input.weight", "_input.bias"}
    assert got["chain"].keys() == got["no_sinks"].keys() and stem < got["chain"].keys()
    assert got["own_rows"].keys() == got["first"].keys() == got["chain"].keys() - stem
    assert len(got["chain"]) == 3 + 2 * 14 + 4
    for route in ("own_rows", "first", "no_sinks"):
        for k, g in got[route].items():
            assert torch.equal(g, got["chain"][k]), f"{route}: gradient of {k} differs from the chain's"


def test_more_than_eight_blocks_take_a_second_launch(dev, lib, monkeypatch):
    """9 blocks under FlatAdam: the stem's backward adds 8 blocks, then the ninth with both ends; the gradients are those of the
    same model without sinks, where every kernel reduces its own rows."""
    from pytorch_generative_amd import ops

    calls = []
    _record_reduces(monkeypatch, lib, calls)
    x = _batch(dev)
    was = ops.set_deterministic(True)
    try:
        chained = _backward(_model(dev, 9), x, sinks=True)
        assert calls == [8, 1], f"pg_gpt_model_reduce calls {calls}"
        plain = _backward(_model(dev, 9), x, sinks=False)
    finally:
        ops.set_deterministic(was)
    assert chained.keys() == plain.keys() and len(chained) == 3 + 9 * 14 + 4
    for k, g in chained.items():
        assert torch.equal(g, plain[k]), f"gradient of {k} differs"
