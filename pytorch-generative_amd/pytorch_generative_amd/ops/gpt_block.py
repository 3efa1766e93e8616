"""ops.gpt_block — the fused position-wise MLP, the ImageGPT block's head / tail kernels (a run of blocks as one autograd node,
and the two halves on their own), the chain of deferred weight-gradient reductions, NCHW LayerNorm.

Part of the operator layer (pytorch_generative_amd.ops): HIP kernels behind torch.autograd.Function, called through the C-ABI
with tensor.data_ptr() and the current stream. No CPU / ATen fallback: a missing library, a CPU tensor or an unsupported shape raises."""

import collections
import ctypes
import os
import weakref

import torch

from pytorch_generative_amd import _lib
from pytorch_generative_amd.ops._common import _chk, _grad_targets, _p, _sink, _stream, zeros, zeros_like
from pytorch_generative_amd.ops.attention import attention_qkv_bwd, attention_qkv_fwd


# --------------------------------------------------------------------------------------------
# fused position-wise MLP (Conv2d 1x1 -> GELU -> Conv2d 1x1 [+ residual])
# --------------------------------------------------------------------------------------------
FUSE_MLP = os.environ.get("PG_FUSE_MLP", "1") != "0"


def mlp_gelu_supported(x, conv1, conv2):
    """The fused kernels are instantiated for the ImageGPT block shape (C = 16 -> 64 -> 16, 1x1,
    L % 16 == 0); anything else runs as conv -> gelu -> conv."""
    if not FUSE_MLP or conv1.bias is None or conv2.bias is None:
        return False
    w1, w2 = conv1.weight, conv2.weight
    return (tuple(w1.shape) == (64, 16, 1, 1) and tuple(w2.shape) == (16, 64, 1, 1)
            and x.shape[1] == 16 and (x.shape[2] * x.shape[3]) % 16 == 0)


class _MlpGelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, res, sinks):
        lib = _lib.load()
        x = _chk(x, "mlp_gelu.x")
        w1, b1, w2, b2 = (_chk(t, "mlp_gelu.param") for t in (w1, b1, w2, b2))
        if res is not None:
            res = _chk(res, "mlp_gelu.res")
        n, c, h, w = x.shape
        y = torch.empty_like(x)
        _lib.check(
            lib.pg_mlp_gelu_fwd(x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                                b2.data_ptr(), _p(res), y.data_ptr(), n, c, w1.shape[0], h * w,
                                _stream()),
            "pg_mlp_gelu_fwd",
        )
        ctx.save_for_backward(x, w1, b1, w2)
        ctx.sinks, ctx.has_res = sinks, res is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, w1, b1, w2 = ctx.saved_tensors
        dy = _chk(dy, "mlp_gelu.dy")
        n, c, h, w = x.shape
        hd = w1.shape[0]
        dx = torch.empty_like(x)
        grads, outs = [], []
        for sink, like in zip(ctx.sinks, (w1, b1, w2, None)):
            if sink is not None:
                grads.append(sink)
                outs.append(None)
            else:
                t = zeros((c,), x.device) if like is None else zeros_like(like)
                grads.append(t)
                outs.append(t)
        ws_n = lib.pg_mlp_gelu_bwd_workspace_floats(n, h * w)
        ws = torch.empty(ws_n, device=x.device, dtype=torch.float32)
        _lib.check(
            lib.pg_mlp_gelu_bwd(x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                                dy.data_ptr(), dx.data_ptr(), grads[0].data_ptr(),
                                grads[1].data_ptr(), grads[2].data_ptr(), grads[3].data_ptr(), n, c,
                                hd, h * w, ws.data_ptr(), ws_n, _stream()),
            "pg_mlp_gelu_bwd",
        )
        return dx, outs[0], outs[1], outs[2], outs[3], (dy if ctx.has_res else None), None


def mlp_gelu(x, conv1, conv2, res=None):
    """res + conv2(gelu(conv1(x))) for two 1x1 convolutions, hidden activations kept in registers
    (check mlp_gelu_supported first)."""
    sinks = (_sink(conv1.weight), _sink(conv1.bias), _sink(conv2.weight), _sink(conv2.bias))
    return _MlpGelu.apply(x, conv1.weight, conv1.bias, conv2.weight, conv2.bias, res, sinks)


# --------------------------------------------------------------------------------------------
# ImageGPT transformer block minus the attention core: fused head / tail (gpt_block.hip)
# --------------------------------------------------------------------------------------------
FUSE_BLOCK = os.environ.get("PG_FUSE_BLOCK", "1") != "0"
# A/B: 0 = tail(i) and head(i+1) as two forward launches instead of pg_gpt_block_tail_head_fwd (read by gpt_blocks per call)
FUSE_BOUNDARY = os.environ.get("PG_FUSE_BOUNDARY", "1") != "0"
# A/B: 0 = head(i+1) and tail(i) as two backward launches instead of pg_gpt_block_head_tail_bwd_partial (read by gpt_blocks per
# call; it concerns only the boundaries that the forward ran fused)
FUSE_BOUNDARY_BWD = os.environ.get("PG_FUSE_BOUNDARY_BWD", "1") != "0"


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def reduce_rows(jobs, n, c, L, out=None, stem=None):
    """Adds partial weight-gradient rows to their destinations (pg_gpt_model_reduce): those of the blocks in `jobs` (as
    _GPTBlocks.backward queues them), 8 blocks per launch, and those of the model's ends, which ride with the last launch
    (the only one when there are no blocks): out = (workspace, rows, Cout, 4 destinations), stem = (workspace, rows, slices, H, W,
    3 destinations). Empties `jobs`."""
    if not jobs and out is None and stem is None:
        return
    lib = _lib.load()
    no_out, no_stem = (0, 0, 0, None), (0, 0, 0, 0, 0, None)
    out_args = no_out if out is None else (out[0].data_ptr(), out[1], out[2], _ptrs(out[3]))
    stem_args = no_stem if stem is None else (stem[0].data_ptr(), *stem[1:5], _ptrs(stem[5]))
    groups = [jobs[i:i + 8] for i in range(0, len(jobs), 8)] or [[]]
    for grp in groups:
        last = grp is groups[-1]
        hw = _ptrs([j[0] for j in grp]) if grp else None
        tw = _ptrs([j[1] for j in grp]) if grp else None
        gr = (ctypes.c_void_p * (14 * len(grp)))(*[ptr for j in grp for ptr in j[2]]) if grp else None
        _lib.check(lib.pg_gpt_model_reduce(len(grp), hw, tw, gr, n, c, L, *(out_args if last else no_out),
                                           *(stem_args if last else no_stem), _stream()), "pg_gpt_model_reduce")
    jobs.clear()


class BlockChain:
    """The deferred weight-gradient reductions of one model's backward pass: `jobs`, one per block whose two backward kernels
    parked their partial rows (_GPTBlocks.backward queues them, last block first), and `out`, the output head's parked rows
    (_GPTOutHead.backward). Whichever backward runs last flushes it: the stem's, else the first block's."""

    def __init__(self):
        self.jobs, self.out = [], None

    def pending(self):
        return len(self.jobs) + (self.out is not None)

    def flush(self, n, c, L, stem=None):
        """Empties the chain: the queued blocks, the output head's rows if its backward parked them, and the caller's stem rows."""
        out, self.out = self.out, None
        reduce_rows(self.jobs, n, c, L, out=out, stem=stem)


_open_chains = []  # weak references to the chains handed out by new_block_chain(): optim.FlatAdam.step() checks that none is pending


def new_block_chain():
    """A BlockChain that assert_no_pending_block_reductions watches."""
    chain = BlockChain()
    _open_chains[:] = [r for r in _open_chains if r() is not None]
    _open_chains.append(weakref.ref(chain))
    return chain


def assert_no_pending_block_reductions():
    """Raises if a backward pass left deferred reductions unflushed (the backward that flushes never ran): the queued
    gradients would silently be missing from the step."""
    for r in _open_chains:
        c = r()
        if c is not None and c.pending():
            raise RuntimeError(f"{c.pending()} deferred ImageGPT weight-gradient reductions were never flushed: the backward "
                               "that flushes them (the stem's, else the first block's) did not run")


# ---- one launch helper per C-ABI entry. head = (ln1 w, ln1 b, wq, bq, wkv, bkv), tail = (wp, bp, ln2 w, ln2 b, w1, b1, w2, b2):
# the parameter order of the kernels' gradient outputs and of the autograd Functions below
def _launch(name, tensors, x, eps, hidden=None, workspaces=()):
    """tensors' pointers, N, C, [hidden,] L, eps, each workspace as (pointer, floats), the current stream"""
    n, c, h, w = x.shape
    dims = (n, c, h * w, eps) if hidden is None else (n, c, hidden, h * w, eps)
    ws = [a for t in workspaces for a in (t.data_ptr(), t.numel())]
    _lib.check(getattr(_lib.load(), name)(*[t.data_ptr() for t in tensors], *dims, *ws, _stream()), name)


def _workspace(kind, x):
    """The partial-row workspace of a block's "head" / "tail" backward kernel."""
    n, _, h, w = x.shape
    floats = getattr(_lib.load(), f"pg_gpt_block_{kind}_bwd_workspace_floats")(n, h * w)
    return torch.empty(floats, device=x.device, dtype=torch.float32)


def _new_qkv(x):
    n, c, h, w = x.shape
    return torch.empty((n, 3 * c, h, w), device=x.device, dtype=torch.float32)


def _head_fwd(x, head, qkv, eps):
    _launch("pg_gpt_block_head_fwd", (x, *head, qkv), x, eps)


def _tail_fwd(o, x, tail, x_new, eps):
    _launch("pg_gpt_block_tail_fwd", (o, x, *tail, x_new), x, eps, tail[4].shape[0])


def _tail_head_fwd(o, x, tail, x_new, head_after, qkv_after, eps):
    """tail_fwd and the FOLLOWING block's head_fwd on x_new in one launch, the same bits; one eps serves both LayerNorms"""
    _launch("pg_gpt_block_tail_head_fwd", (o, x, *tail, x_new, *head_after, qkv_after), x, eps, tail[4].shape[0])


def _head_bwd_inputs(x, head, dqkv, gx):
    lnw, lnb, wq, _, wkv, _ = head
    return (x, lnw, lnb, wq, wkv, dqkv, gx)


def _head_bwd(x, head, dqkv, gx, dx, eps, ws, grads=()):
    """grads: the six destinations, added to by the kernel's own reduction; without them the partial rows stay in ws"""
    _launch("pg_gpt_block_head_bwd" if grads else "pg_gpt_block_head_bwd_partial",
            (*_head_bwd_inputs(x, head, dqkv, gx), dx, *grads), x, eps, workspaces=(ws,))


def _tail_bwd(o, x, tail, d, d_o, gx, eps, ws, grads=()):
    """grads: the eight destinations; without them the partial rows stay in ws"""
    _launch("pg_gpt_block_tail_bwd" if grads else "pg_gpt_block_tail_bwd_partial",
            (o, x, *tail[:7], d, d_o, gx, *grads), x, eps, tail[4].shape[0], (ws,))


def _head_tail_bwd_partial(head_inputs, o, x, tail, d_o, gx, eps, head_ws, ws):
    """head_bwd_partial of the FOLLOWING block (head_inputs: its _head_bwd_inputs) and tail_bwd_partial on the dx it would have
    written, in one launch: that dx stays in registers"""
    _launch("pg_gpt_block_head_tail_bwd_partial", (*head_inputs, o, x, *tail[:7], d_o, gx), x, eps, tail[4].shape[0],
            (head_ws, ws))


# ---- the stand-alone halves (the K/V-cached sampler runs them around pg_attn_decode); each backward reduces its own rows
class _GPTBlockHead(torch.autograd.Function):
    """(qkv, x) = ([W_q; W_kv] LN1(x) + b, x). The second output aliases x: whatever gradient reaches it
    (the residual routes of the block) is added to LN1's input gradient inside the backward kernel."""

    @staticmethod
    def forward(ctx, x, lnw, lnb, wq, bq, wkv, bkv, eps, params):
        x_in = x
        x = _chk(x, "gpt_block_head.x")
        qkv = _new_qkv(x)
        _head_fwd(x, (lnw, lnb, wq, bq, wkv, bkv), qkv, eps)
        ctx.save_for_backward(x, lnw, lnb, wq, bq, wkv, bkv)
        ctx.eps, ctx.params = eps, params
        return qkv, x_in

    @staticmethod
    def backward(ctx, dqkv, gx):
        x, *head = ctx.saved_tensors
        if dqkv is None:
            return gx, None, None, None, None, None, None, None, None
        dqkv = _chk(dqkv, "gpt_block_head.dqkv")
        gx = zeros_like(x) if gx is None else _chk(gx, "gpt_block_head.gx")
        dx = torch.empty_like(x)
        tgt, ret = _grad_targets(ctx.params)
        _head_bwd(x, head, dqkv, gx, dx, ctx.eps, _workspace("head", x), tgt)
        return (dx, *ret, None, None)


class _LastTail:
    """What the backward of the tail node behind a run of blocks (gpt_blocks) hands to the run's backward, which runs next: o,
    which both read and the run then need not save, and — if the tail parked them — its partial rows, which the run makes one
    job with the last head's: rows = (workspace, the 8 destinations)."""
    __slots__ = ("o", "rows")

    def __init__(self):
        self.o = self.rows = None


class _GPTBlockTail(torch.autograd.Function):
    """x_new = x + x_mid + mlp(LN2(x_mid)), x_mid = x + W_p o + b_p (projection, both residuals of the
    block and the model loop's `x + block(x)`). park: a _LastTail — the backward then leaves its partial rows there instead of
    reducing them, if every parameter has a sink."""

    @staticmethod
    def forward(ctx, o, x, wp, bp, lnw, lnb, w1, b1, w2, b2, eps, params, park=None):
        o = _chk(o, "gpt_block_tail.o")
        x = _chk(x, "gpt_block_tail.x")
        x_new = torch.empty_like(x)
        _tail_fwd(o, x, (wp, bp, lnw, lnb, w1, b1, w2, b2), x_new, eps)
        ctx.save_for_backward(o, x, wp, bp, lnw, lnb, w1, b1, w2, b2)
        ctx.eps, ctx.params, ctx.park = eps, params, park
        return x_new

    @staticmethod
    def backward(ctx, d):
        o, x, *tail = ctx.saved_tensors
        tgt, ret = _grad_targets(ctx.params)
        d = _chk(d, "gpt_block_tail.dx_new")
        d_o, gx = torch.empty_like(o), torch.empty_like(x)
        ws = _workspace("tail", x)
        parks = ctx.park is not None and all(r is None for r in ret)
        _tail_bwd(o, x, tail, d, d_o, gx, ctx.eps, ws, () if parks else tgt)
        if ctx.park is not None:
            ctx.park.o, ctx.park.rows = o, (ws, tgt) if parks else None
        return (d_o, gx, *ret, None, None, None)


def gpt_block_supported(x, ln1, q, kv, proj, ln2, fc1, fc2):
    """The fused block kernels cover the BASELINE.json ImageGPT block: 16 channels, 1x1 projections
    with biases, 64 hidden units, L % 16 == 0."""
    if not FUSE_BLOCK or x.shape[1] != 16 or (x.shape[2] * x.shape[3]) % 16 != 0:
        return False
    shapes = (tuple(q.weight.shape), tuple(kv.weight.shape), tuple(proj.weight.shape),
              tuple(fc1.weight.shape), tuple(fc2.weight.shape))
    if shapes != ((16, 16, 1, 1), (32, 16, 1, 1), (16, 16, 1, 1), (64, 16, 1, 1), (16, 64, 1, 1)):
        return False
    if any(m.bias is None for m in (q, kv, proj, fc1, fc2)):
        return False
    return tuple(ln1.normalized_shape) == (16,) and tuple(ln2.normalized_shape) == (16,)


def gpt_block_head(x, ln1, q, kv):
    params = (ln1.weight, ln1.bias, q.weight, q.bias, kv.weight, kv.bias)
    return _GPTBlockHead.apply(x, *params, float(ln1.eps), params)


def gpt_block_tail(o, x, proj, ln2, fc1, fc2):
    params = (proj.weight, proj.bias, ln2.weight, ln2.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias)
    return _GPTBlockTail.apply(o, x, *params, float(ln2.eps), params)


# ---- a run of consecutive blocks as ONE autograd node: both sides of every block boundary are in sight, so the boundary kernels
# need no protocol. What is launched is decided by the two planners below, which touch no tensor.
def plan_blocks_forward(fusable):
    """The block-kernel launches of a forward over len(fusable) + 1 blocks, in order (each block's attention runs in front of
    its tail). fusable[i]: the boundary between blocks i and i + 1 may run as one launch."""
    steps = [("head_fwd", 0)]
    for i, fuse in enumerate(fusable):
        steps += [("tail_head_fwd", i, i + 1)] if fuse else [("tail_fwd", i), ("head_fwd", i + 1)]
    return steps + [("tail_fwd", len(fusable))]


def plan_blocks_backward(tail_sunk, head_sunk, fused, chain=False, flush=False, fuse_bwd=True, queued=0, first=0):
    """The block-kernel launches and reductions of a backward over blocks first .. len(tail_sunk) - 1, last block first:
    [(i, steps up to block i's attention backward, steps after it)], a step = (name, block indices ... or a count).

    tail_sunk[i] / head_sunk[i]: every tail / head parameter of block i has a gradient sink; fused[i]: the forward ran the
    boundary between blocks i and i + 1 as one launch; chain: a BlockChain collects the blocks' jobs, `queued` of them are in
    it already; flush: block 0 of this run empties the chain; fuse_bwd: FUSE_BOUNDARY_BWD.

    A tail whose parameters all have sinks parks its partial rows (tail_bwd_partial), and so does the head after it
    (head_bwd_partial): the two workspaces are one job, reduced at once ("reduce_block") or — with a chain, when the head's
    parameters all have sinks too — queued ("queue") for whoever flushes ("reduce_queue", n: the n oldest jobs, at most 8 per
    launch). A queued head behind a boundary that the forward ran fused leaves its launch to the tail of the block below, which
    runs both in one kernel (head_tail_bwd_partial) if it parks as well, and else runs the head's launch first, on its own.
    Any other tail and the head after it reduce their own rows (tail_bwd, head_bwd)."""
    def reduce_queue():
        return [("reduce_queue", min(8, queued - j)) for j in range(0, queued, 8)]

    visits, left = [], False  # left: the head launch of block i + 1 is still to run
    for i in reversed(range(first, len(tail_sunk))):
        parked = tail_sunk[i]
        if parked:
            tail = [("head_tail_bwd_partial", i + 1, i) if left else ("tail_bwd_partial", i)]
        else:
            tail = [("head_bwd_partial", i + 1)] * left + [("tail_bwd", i)]
        queue = bool(parked and chain and head_sunk[i])
        flusher = bool(chain and flush and i == 0)
        head = []
        if flusher and queued and not queue:  # this block reduces its own rows: the others' still must not wait
            head, queued = reduce_queue(), 0
        left = bool(queue and i > first and fused[i - 1] and fuse_bwd)
        if not parked:
            head.append(("head_bwd", i))
        elif left:
            head.append(("queue", i))  # the head rows are written before anyone reduces the job: tail(i - 1) runs first
            queued += 1
        else:
            head.append(("head_bwd_partial", i))
            head.append(("queue", i) if queue else ("reduce_block", i))
            queued += queue
            if queue and flusher:
                head, queued = head + reduce_queue(), 0
        visits.append((i, tail, head))
    return visits


class _GPTBlocks(torch.autograd.Function):
    """A run of k fused-shape blocks up to the attention of the last: (o, x) of block k - 1, for the _GPTBlockTail node that
    gpt_blocks puts behind it. That tail is a node of its own so that d x_k, which only its kernel reads, dies with it: autograd
    holds a node's incoming gradients until the node returns. Inputs: x, the run's description, then per block 6 head and 8
    tail parameters, the last block's tail parameters left out."""

    @staticmethod
    def forward(ctx, x, run, *params):
        x = x0 = _chk(x, "gpt_blocks.x")
        blocks = [params[i:i + 14] for i in range(0, len(params), 14)]
        kept, qkv = [], None
        for op, i, *_ in plan_blocks_forward(run.fusable)[:-1]:
            eps1, eps2, attn = run.blocks[i]
            if op == "head_fwd":
                qkv = _new_qkv(x)
                _head_fwd(x, blocks[i][:6], qkv, eps1)
                continue
            o, lse2 = attention_qkv_fwd(qkv, *attn)
            if run.keep:  # x_0 is saved below
                kept.append((x if i else None, qkv, o, lse2))
            x_new = torch.empty_like(x)
            if op == "tail_fwd":
                _tail_fwd(o, x, blocks[i][6:], x_new, eps2)
            else:
                qkv = _new_qkv(x)
                _tail_head_fwd(o, x, blocks[i][6:], x_new, blocks[i + 1][:6], qkv, eps2)
            x = x_new
        o, lse2 = attention_qkv_fwd(qkv, *run.blocks[-1][2])
        ctx.save_for_backward(x0, x, *params)  # o reaches backward through run.park: it is freed after its last reader there
        # the other tensors made here are kept per block, so that backward lets go of a block's as soon as it is done with them
        ctx.run, ctx.params, ctx.kept = run, params, kept + [(qkv, lse2)] if run.keep else None
        return o, x

    @staticmethod
    def backward(ctx, d_o, gx):
        x0, x_last, *data = ctx.saved_tensors
        run, kept, ctx.kept = ctx.run, ctx.kept, None
        if kept is None:
            raise RuntimeError("gpt_blocks: backward ran a second time; the activations were released by the first")
        chain = run.chain
        k, (n, c, h, w) = len(run.blocks), x0.shape
        params = [ctx.params[14 * i:14 * i + 14] for i in range(k)]  # the Parameter objects: they carry the sinks
        sunk = lambda ps: all(_sink(p) is not None for p in ps)  # noqa: E731
        park = run.park  # from the tail node, whose backward ran in front of this one
        o_last, last_rows, park.o, park.rows = park.o, park.rows, None, None
        tail_sunk = [sunk(p[6:]) for p in params[:-1]] + [last_rows is not None]
        needs = ctx.needs_input_grad
        # nothing below block `first` needs a gradient. (Block `first` runs whole, its head included, even where only its tail
        # does: autograd would have pruned that head; the results are the same.)
        first = 0 if needs[0] else min(i for i in range(k) if any(needs[2 + 14 * i:16 + 14 * i]))
        visits = plan_blocks_backward(tail_sunk, [sunk(p[:6]) for p in params], run.fusable, chain is not None, run.flush,
                                      run.fuse_bwd, len(chain.jobs) if chain else 0, first)
        d_o, gx = _chk(d_o, "gpt_blocks.d_o"), _chk(gx, "gpt_blocks.gx")
        rets = [[None] * len(p) for p in params]
        left = d = None  # left: (x, head, dqkv, gx), (eps, workspace) of the block above while its head launch is still to run
        for i, tail_steps, head_steps in visits:
            eps1, eps2, attn = run.blocks[i]
            head, tail = data[14 * i:14 * i + 6], data[14 * i + 6:14 * i + 14]
            if i == k - 1:  # its tail steps ran in the node in front of this one
                (qkv, lse2), x, o, o_last = kept.pop(), x_last, o_last, None
                t_ws, t_tgt = last_rows or (None, None)
                t_ret = []
            else:
                x, qkv, o, lse2 = kept.pop()
                x = x0 if i == 0 else x
                t_tgt, t_ret = _grad_targets(params[i][6:])
                d_o, gx = torch.empty_like(o), torch.empty_like(x)
            for op, *_ in tail_steps if i < k - 1 else ():
                if op == "head_bwd_partial":  # this tail reduces its own rows: the launch left to it runs on its own after all
                    d = torch.empty_like(x)
                    _head_bwd(*left[0], d, *left[1])
                    continue
                t_ws = _workspace("tail", x)
                if op == "head_tail_bwd_partial":
                    _head_tail_bwd_partial(_head_bwd_inputs(*left[0]), o, x, tail, d_o, gx, eps2, left[1][1], t_ws)
                else:
                    _tail_bwd(o, x, tail, d, d_o, gx, eps2, t_ws, () if op == "tail_bwd_partial" else t_tgt)
            left = d = None  # as between autograd nodes: nothing outlives its last reader
            dqkv = attention_qkv_bwd(qkv, o, lse2, d_o, *attn)
            del qkv, o, lse2, d_o
            h_tgt, h_ret = _grad_targets(params[i][:6])
            h_ws = _workspace("head", x)
            # 14 destinations in the order of pg_gpt_model_reduce: head | tail w1, b1, w2, b2, wp, bp, ln2 w, ln2 b
            job = tail_sunk[i] and (h_ws, t_ws, [g.data_ptr() for g in h_tgt + t_tgt[4:] + t_tgt[:4]], (h_tgt, t_tgt))
            for op, arg in head_steps:
                if op == "reduce_queue":
                    oldest = chain.jobs[:arg]
                    del chain.jobs[:arg]
                    reduce_rows(oldest, n, c, h * w)
                elif op == "reduce_block":
                    reduce_rows([job], n, c, h * w)
                elif op == "queue":
                    chain.jobs.append(job)
                else:
                    d = torch.empty_like(x)
                    _head_bwd(x, head, dqkv, gx, d, eps1, h_ws, h_tgt if op == "head_bwd" else ())
            if d is None:  # queued only: the launch is left to the tail of the block below, which has d in registers
                left = ((x, head, dqkv, gx), (eps1, h_ws))
            del dqkv, gx
            rets[i] = h_ret + t_ret
        return (d, None, *[g for r in rets for g in r])


_Run = collections.namedtuple("_Run", "blocks fusable chain flush fuse_bwd keep park")


def gpt_blocks(x, blocks, chain=None, flush=False):
    """x + block(x), block after block, for consecutive ImageGPT blocks (models.image_gpt.TransformerBlock; each must pass
    gpt_block_supported: TransformerBlock._fused_ok) as one autograd node and the last block's tail behind it. Forward: head(0),
    then per block the attention core and one launch for its tail and the next block's head (two with FUSE_BOUNDARY off or
    differing LayerNorm eps). Backward: the blocks in reverse, launches and reductions by plan_blocks_backward; it releases the
    activations as it goes, so a second backward over the same graph (retain_graph=True) raises.
    chain: the model's BlockChain (new_block_chain) — the jobs of the blocks are queued there for ONE reduction launch per 8
    blocks by whoever flushes it; flush: this run's first block is the model's first and nothing behind it (a stem) flushes."""
    specs, params = [], []
    for blk in blocks:
        a = blk._attn
        params += [blk._ln1.weight, blk._ln1.bias, a._q.weight, a._q.bias, a._kv.weight, a._kv.bias, a._proj.weight, a._proj.bias,
                   blk._ln2.weight, blk._ln2.bias, blk._out[0].weight, blk._out[0].bias, blk._out[2].weight, blk._out[2].bias]
        specs.append((float(blk._ln1.eps), float(blk._ln2.eps),
                      (a._n_heads, a._embed_channels, a._out_channels, bool(a._mask_center))))
    params, last_tail = params[:-8], tuple(params[-8:])
    fusable = [FUSE_BOUNDARY and lo[1] == hi[0] for lo, hi in zip(specs, specs[1:])]
    keep = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
    park = _LastTail() if keep else None  # only a run whose backward will come may be left rows
    o, xs = _GPTBlocks.apply(x, _Run(specs, fusable, chain, bool(flush), FUSE_BOUNDARY_BWD, keep, park), *params)
    return _GPTBlockTail.apply(o, xs, *last_tail, specs[-1][1], last_tail, park)


# --------------------------------------------------------------------------------------------
# NCHW LayerNorm
# --------------------------------------------------------------------------------------------
class _NCHWLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, gg, gb, with_skip=False):
        lib = _lib.load()
        x_in = x
        x = _chk(x, "layernorm.x")
        n, c, h, w = x.shape
        if gamma.numel() != c:
            raise ValueError(f"NCHWLayerNorm: normalized_shape {gamma.numel()} != channels {c}")
        y = torch.empty_like(x)
        mean = torch.empty(n * h * w, device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        _lib.check(
            lib.pg_nchw_layernorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
                                      mean.data_ptr(), rstd.data_ptr(), n, c, h * w, eps, _stream()),
            "pg_nchw_layernorm_fwd",
        )
        ctx.save_for_backward(x, gamma, mean, rstd)
        ctx.gg, ctx.gb = gg, gb
        if with_skip:
            # second output: x itself (autograd aliases it). Whatever gradient reaches x through this
            # alias — the residual branch of `x + f(LN(x))` — is added in the backward kernel's
            # epilogue instead of by a separate accumulation pass over the activation.
            return y, x_in
        return y

    @staticmethod
    def backward(ctx, dy, dskip=None):
        lib = _lib.load()
        x, gamma, mean, rstd = ctx.saved_tensors
        if dy is None:  # only the skip output was used
            return dskip, None, None, None, None, None, None
        dy = _chk(dy, "layernorm.dy")
        n, c, h, w = x.shape
        dx = torch.empty_like(x)
        dg = db = None
        gg, gb = ctx.gg, ctx.gb
        if gg is None:
            dg = zeros((c,), x.device)
            gg = dg
        if gb is None:
            db = zeros((c,), x.device)
            gb = db
        ws_n = lib.pg_nchw_layernorm_bwd_workspace_floats(n, c, h * w)
        ws = torch.empty(ws_n, device=x.device, dtype=torch.float32)
        if dskip is None:
            _lib.check(
                lib.pg_nchw_layernorm_bwd(x.data_ptr(), gamma.data_ptr(), mean.data_ptr(),
                                          rstd.data_ptr(), dy.data_ptr(), dx.data_ptr(), gg.data_ptr(),
                                          gb.data_ptr(), n, c, h * w, ws.data_ptr(), ws_n, _stream()),
                "pg_nchw_layernorm_bwd",
            )
        else:
            dskip = _chk(dskip, "layernorm.dskip")
            _lib.check(
                lib.pg_nchw_layernorm_bwd_res(x.data_ptr(), gamma.data_ptr(), mean.data_ptr(),
                                              rstd.data_ptr(), dy.data_ptr(), dskip.data_ptr(),
                                              dx.data_ptr(), gg.data_ptr(), gb.data_ptr(), n, c,
                                              h * w, ws.data_ptr(), ws_n, _stream()),
                "pg_nchw_layernorm_bwd_res",
            )
        return dx, dg, db, None, None, None, None


def nchw_layernorm(x, weight, bias, eps=1e-5):
    return _NCHWLayerNorm.apply(x, weight, bias, float(eps), _sink(weight), _sink(bias))


def nchw_layernorm_skip(x, weight, bias, eps=1e-5):
    """(LN(x), x): use the second output for the residual branch of `x + f(LN(x))`; its gradient is
    then added to LN's input gradient inside the backward kernel."""
    return _NCHWLayerNorm.apply(x, weight, bias, float(eps), _sink(weight), _sink(bias), True)
