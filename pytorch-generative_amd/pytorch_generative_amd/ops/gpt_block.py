"""ops.gpt_block — the fused position-wise MLP, the ImageGPT block's head / tail kernels, NCHW LayerNorm.

Part of the operator layer (pytorch_generative_amd.ops): HIP kernels behind torch.autograd.Function, called through the C-ABI
with tensor.data_ptr() and the current stream. No CPU / ATen fallback: a missing library, a CPU tensor or an unsupported shape raises."""

import ctypes
import os

import torch

from pytorch_generative_amd import _lib
from pytorch_generative_amd.ops._common import _chk, _p, _sink, _stream, zeros, zeros_like


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
# A/B: 0 = tail(i) and head(i+1) as two forward launches instead of pg_gpt_block_tail_head_fwd (read by ImageGPT.forward per call)
FUSE_BOUNDARY = os.environ.get("PG_FUSE_BOUNDARY", "1") != "0"
# A/B: 0 = head(i+1) and tail(i) as two backward launches instead of pg_gpt_block_head_tail_bwd_partial (read by ImageGPT.forward per
# call; it concerns only the boundaries that the forward ran fused)
FUSE_BOUNDARY_BWD = os.environ.get("PG_FUSE_BOUNDARY_BWD", "1") != "0"


def _grad_targets(params):
    """Per parameter: (tensor the kernel adds into, value to return to autograd): the direct sink if
    the parameter has one (then autograd gets None), else a fresh zero tensor."""
    tgt, ret = [], []
    for p in params:
        sink = _sink(p)
        if sink is not None:
            tgt.append(sink)
            ret.append(None)
        else:
            z = zeros_like(p)
            tgt.append(z)
            ret.append(z)
    return tgt, ret


_open_chains = []  # weak references to the queues handed out by new_block_chain(): optim.FlatAdam.step() checks that none is pending


def new_block_chain():
    """A queue for the deferred weight-gradient reductions of a model's blocks (see gpt_block_head)."""
    import weakref

    class _Chain(dict):
        pass

    chain = _Chain(jobs=[])
    _open_chains[:] = [r for r in _open_chains if r() is not None]
    _open_chains.append(weakref.ref(chain))
    return chain


def assert_no_pending_block_reductions():
    """Raises if a backward pass left deferred reductions unflushed (the block that flushes never ran backward): the queued
    gradients would silently be missing from the step."""
    for r in _open_chains:
        c = r()
        if c is not None and (c["jobs"] or c.get("out") is not None):
            raise RuntimeError(f"{len(c['jobs']) + (c.get('out') is not None)} deferred ImageGPT weight-gradient reductions were "
                               "never flushed: the backward that flushes them (the stem's, else the first block's) did not run")
        if c is not None and c.get("deferred") is not None:
            raise RuntimeError("a deferred ImageGPT head backward launch never ran: the backward of the previous block's tail, "
                               "which takes it, did not run")


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def reduce_rows(jobs, n, c, L, out=None, stem=None):
    """Adds partial weight-gradient rows to their destinations (pg_gpt_model_reduce): those of the blocks in `jobs` (as
    _GPTBlockHead.backward queues them), 8 blocks per launch, and those of the model's ends, which ride with the last launch
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


def _take_boundary_qkv(pair, x, head, eps):
    """The qkv that the previous block's tail already computed for exactly this input (pg_gpt_block_tail_head_fwd), or None.
    The entry is keyed by the tail's x_new: it is taken only for the same memory at the same version, with the same six
    parameter tensors and eps, and it is removed whether it matches or not."""
    boundary = pair.get("boundary") if pair is not None else None
    entry = boundary.pop("qkv", None) if boundary is not None else None
    if entry is None:
        return None
    x_new, version, params, e, qkv = entry
    same = (x.data_ptr() == x_new.data_ptr() and x.shape == x_new.shape and x.stride() == x_new.stride()
            and x._version == version and e == eps and len(params) == len(head) and all(a is b for a, b in zip(params, head)))
    return qkv if same else None


def _pop_deferred_head(pair):
    """The head backward launch that the NEXT block's _GPTBlockHead.backward left to this block's tail (pair["boundary"]["bwd"]),
    or None. It is removed; whoever pops it launches it, fused or on its own."""
    boundary = pair.get("boundary") if pair is not None else None
    entry = boundary.pop("bwd", None) if boundary is not None else None
    if entry is not None:
        entry["chain"]["deferred"] = None
    return entry


def _is_deferred_dx(d, entry):
    """d is the very tensor the deferred head backward returned unwritten: same memory, shape, strides and version."""
    dx = entry["dx"]
    return (d.data_ptr() == dx.data_ptr() and d.shape == dx.shape and d.stride() == dx.stride() and d.dtype == dx.dtype
            and d._version == entry["version"])


def _launch_deferred_head(entry):
    """The deferred launch on its own, as _GPTBlockHead.backward would have run it: writes entry["dx"]."""
    x, lnw, lnb, wq, wkv, dqkv, gx = entry["head"]
    ws, (n, c, L) = entry["ws"], entry["geometry"]
    _lib.check(_lib.load().pg_gpt_block_head_bwd_partial(x.data_ptr(), lnw.data_ptr(), lnb.data_ptr(), wq.data_ptr(),
                                                         wkv.data_ptr(), dqkv.data_ptr(), gx.data_ptr(), entry["dx"].data_ptr(),
                                                         n, c, L, entry["eps"], ws.data_ptr(), ws.numel(), _stream()),
               "pg_gpt_block_head_bwd_partial")


class _GPTBlockHead(torch.autograd.Function):
    """(qkv, x) = ([W_q; W_kv] LN1(x) + b, x). The second output aliases x: whatever gradient reaches it
    (the residual routes of the block) is added to LN1's input gradient inside the backward kernel."""

    @staticmethod
    def forward(ctx, x, lnw, lnb, wq, bq, wkv, bkv, eps, params, pair=None):
        lib = _lib.load()
        ctx.pair = pair
        x_in = x
        x = _chk(x, "gpt_block_head.x")
        n, c, h, w = x.shape
        qkv = _take_boundary_qkv(pair, x, (lnw, lnb, wq, bq, wkv, bkv), eps)
        # the backward may leave its launch to the previous block's tail only where that tail ran this head in its forward launch and
        # the caller vouches that x has no other consumer (pair["defer_bwd"], set by ImageGPT.forward)
        ctx.defer = qkv is not None and bool(pair.get("defer_bwd"))
        if qkv is None:
            qkv = torch.empty((n, 3 * c, h, w), device=x.device, dtype=torch.float32)
            _lib.check(
                lib.pg_gpt_block_head_fwd(x.data_ptr(), lnw.data_ptr(), lnb.data_ptr(), wq.data_ptr(),
                                          bq.data_ptr(), wkv.data_ptr(), bkv.data_ptr(), qkv.data_ptr(),
                                          n, c, h * w, eps, _stream()),
                "pg_gpt_block_head_fwd",
            )
        ctx.save_for_backward(x, lnw, lnb, wq, wkv)
        ctx.eps, ctx.params = eps, params
        return qkv, x_in

    @staticmethod
    def backward(ctx, dqkv, gx):
        lib = _lib.load()
        x, lnw, lnb, wq, wkv = ctx.saved_tensors
        n, c, h, w = x.shape
        pending = ctx.pair.pop("tail", None) if ctx.pair is not None else None
        chain = ctx.pair.get("chain") if ctx.pair is not None else None
        flusher = chain is not None and bool(ctx.pair.get("flush"))
        if dqkv is None:
            if flusher and chain["jobs"]:  # the other blocks' rows must not wait for a path this backward does not take
                reduce_rows(chain["jobs"], n, c, h * w)
            if pending is not None:
                raise RuntimeError("gpt_block_head: a deferred tail reduction is pending but the head has no gradient")
            return gx, None, None, None, None, None, None, None, None, None
        dqkv = _chk(dqkv, "gpt_block_head.dqkv")
        gx = zeros_like(x) if gx is None else _chk(gx, "gpt_block_head.gx")
        dx = torch.empty_like(x)
        tgt, ret = _grad_targets(ctx.params)  # order: lnw, lnb, wq, bq, wkv, bkv
        ws_n = lib.pg_gpt_block_head_bwd_workspace_floats(n, h * w)
        ws = torch.empty(ws_n, device=x.device, dtype=torch.float32)
        head_args = (x.data_ptr(), lnw.data_ptr(), lnb.data_ptr(), wq.data_ptr(),
                     wkv.data_ptr(), dqkv.data_ptr(), gx.data_ptr(), dx.data_ptr())
        geometry = (n, c, h * w, ctx.eps, ws.data_ptr(), ws_n, _stream())
        queue = pending is not None and chain is not None and all(r is None for r in ret)
        if flusher and chain["jobs"] and not queue:  # this block reduces its own rows (a parameter without a sink): still flush the others'
            reduce_rows(chain["jobs"], n, c, h * w)
        if pending is None:
            _lib.check(lib.pg_gpt_block_head_bwd(*head_args, *(g.data_ptr() for g in tgt), *geometry), "pg_gpt_block_head_bwd")
            return (dx, *ret, None, None, None)
        # this block's tail kernel left its partial rows: the head kernel leaves its own as well, and both are one job. On a
        # model-level chain of blocks (ImageGPT passes one to all of its blocks) whose every head parameter has a sink the job
        # waits for the LAST backward of the model, which adds the rows of every block with one launch per 8 blocks; otherwise
        # it is reduced at once, one launch for the block
        t_ws, t = pending  # t order: wp, bp, lnw, lnb, w1, b1, w2, b2
        # 14 destinations in the C-ABI's order: head lnw, lnb, wq, bq, wkv, bkv | tail w1, b1, w2, b2, wp, bp, lnw, lnb
        job = (ws, t_ws, [g.data_ptr() for g in tgt + t[4:] + t[:4]], (tgt, t))
        if queue and not flusher and ctx.defer:
            # The launch is left to the previous block's tail backward, which receives dx as its d x_new and runs both chains in one
            # kernel (pg_gpt_block_head_tail_bwd_partial): dx is returned unwritten and is never read if that happens. The job is
            # queued now, as always; its head rows are written before the model's last backward reduces them.
            entry = {"dx": dx, "version": dx._version, "head": (x, lnw, lnb, wq, wkv, dqkv, gx), "ws": ws,
                     "geometry": (n, c, h * w), "eps": ctx.eps, "chain": chain}
            ctx.pair["boundary"]["bwd"] = chain["deferred"] = entry
            chain["jobs"].append(job)
            return (dx, *ret, None, None, None)
        _lib.check(lib.pg_gpt_block_head_bwd_partial(*head_args, *geometry), "pg_gpt_block_head_bwd_partial")
        if not queue:
            reduce_rows([job], n, c, h * w)
        else:
            chain["jobs"].append(job)
            if flusher:
                reduce_rows(chain["jobs"], n, c, h * w)
        return (dx, *ret, None, None, None)


class _GPTBlockTail(torch.autograd.Function):
    """x_new = x + x_mid + mlp(LN2(x_mid)), x_mid = x + W_p o + b_p (projection, both residuals of the
    block and the model loop's `x + block(x)`)."""

    @staticmethod
    def forward(ctx, o, x, wp, bp, lnw, lnb, w1, b1, w2, b2, eps, params, pair=None):
        lib = _lib.load()
        ctx.pair = pair
        # optional: the six parameter tensors of the NEXT block's head (gpt_block_tail), used as raw pointers only
        next_head = pair.pop("next_head", None) if pair is not None else None
        o = _chk(o, "gpt_block_tail.o")
        x = _chk(x, "gpt_block_tail.x")
        n, c, h, w = x.shape
        x_new = torch.empty_like(x)
        if next_head is not None:
            # the next block's head in the same launch: its qkv waits in pair["boundary"] for that block's _GPTBlockHead.forward,
            # which returns it as its own output (autograd sees the same graph as with two launches); next_head's tensors are
            # raw pointers here, their gradients come from the next head's backward as always
            qkv = torch.empty((n, 3 * c, h, w), device=x.device, dtype=torch.float32)
            _lib.check(
                lib.pg_gpt_block_tail_head_fwd(o.data_ptr(), x.data_ptr(), wp.data_ptr(), bp.data_ptr(),
                                               lnw.data_ptr(), lnb.data_ptr(), w1.data_ptr(), b1.data_ptr(),
                                               w2.data_ptr(), b2.data_ptr(), x_new.data_ptr(),
                                               *(t.data_ptr() for t in next_head), qkv.data_ptr(), n, c,
                                               w1.shape[0], h * w, eps, _stream()),
                "pg_gpt_block_tail_head_fwd",
            )
            pair["boundary"]["qkv"] = (x_new, x_new._version, tuple(next_head), eps, qkv)
        else:
            _lib.check(
                lib.pg_gpt_block_tail_fwd(o.data_ptr(), x.data_ptr(), wp.data_ptr(), bp.data_ptr(),
                                          lnw.data_ptr(), lnb.data_ptr(), w1.data_ptr(), b1.data_ptr(),
                                          w2.data_ptr(), b2.data_ptr(), x_new.data_ptr(), n, c,
                                          w1.shape[0], h * w, eps, _stream()),
                "pg_gpt_block_tail_fwd",
            )
        ctx.save_for_backward(o, x, wp, bp, lnw, lnb, w1, b1, w2)
        ctx.eps, ctx.params = eps, params
        return x_new

    @staticmethod
    def backward(ctx, d):
        lib = _lib.load()
        o, x, wp, bp, lnw, lnb, w1, b1, w2 = ctx.saved_tensors
        n, c, h, w = x.shape
        tgt, ret = _grad_targets(ctx.params)  # order: wp, bp, lnw, lnb, w1, b1, w2, b2
        parks = ctx.pair is not None and all(r is None for r in ret)
        # the next block's head backward may have left its launch to this one: taken only if d is the tensor it returned unwritten
        # and this kernel parks its rows as well; otherwise that launch runs first, on its own, and d is then what it wrote
        deferred = _pop_deferred_head(ctx.pair)
        fuse = (deferred is not None and parks and _is_deferred_dx(d, deferred) and deferred["eps"] == ctx.eps
                and deferred["geometry"] == (n, c, h * w))
        if deferred is not None and not fuse:
            _launch_deferred_head(deferred)
        d = _chk(d, "gpt_block_tail.dx_new")
        d_o, gx = torch.empty_like(o), torch.empty_like(x)
        ws_n = lib.pg_gpt_block_tail_bwd_workspace_floats(n, h * w)
        ws = torch.empty(ws_n, device=x.device, dtype=torch.float32)
        if fuse:
            hws = deferred["ws"]
            _lib.check(
                lib.pg_gpt_block_head_tail_bwd_partial(*(t.data_ptr() for t in deferred["head"]), o.data_ptr(), x.data_ptr(),
                                                       wp.data_ptr(), bp.data_ptr(), lnw.data_ptr(), lnb.data_ptr(),
                                                       w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), d_o.data_ptr(), gx.data_ptr(),
                                                       n, c, w1.shape[0], h * w, ctx.eps, hws.data_ptr(), hws.numel(),
                                                       ws.data_ptr(), ws_n, _stream()),
                "pg_gpt_block_head_tail_bwd_partial",
            )
            ctx.pair["tail"] = (ws, tgt)
            return (d_o, gx, *ret, None, None, None)
        if parks:
            # every gradient goes into a sink (FlatAdam): leave the partial rows for the head's backward of the
            # same block, which reduces both kernels' rows in one launch or queues them for the model's
            _lib.check(
                lib.pg_gpt_block_tail_bwd_partial(o.data_ptr(), x.data_ptr(), wp.data_ptr(), bp.data_ptr(),
                                                  lnw.data_ptr(), lnb.data_ptr(), w1.data_ptr(), b1.data_ptr(),
                                                  w2.data_ptr(), d.data_ptr(), d_o.data_ptr(), gx.data_ptr(), n, c,
                                                  w1.shape[0], h * w, ctx.eps, ws.data_ptr(), ws_n, _stream()),
                "pg_gpt_block_tail_bwd_partial",
            )
            ctx.pair["tail"] = (ws, tgt)
            return (d_o, gx, *ret, None, None, None)
        _lib.check(
            lib.pg_gpt_block_tail_bwd(o.data_ptr(), x.data_ptr(), wp.data_ptr(), bp.data_ptr(),
                                      lnw.data_ptr(), lnb.data_ptr(), w1.data_ptr(), b1.data_ptr(),
                                      w2.data_ptr(), d.data_ptr(), d_o.data_ptr(), gx.data_ptr(),
                                      tgt[0].data_ptr(), tgt[1].data_ptr(), tgt[2].data_ptr(),
                                      tgt[3].data_ptr(), tgt[4].data_ptr(), tgt[5].data_ptr(),
                                      tgt[6].data_ptr(), tgt[7].data_ptr(), n, c, w1.shape[0], h * w,
                                      ctx.eps, ws.data_ptr(), ws_n, _stream()),
            "pg_gpt_block_tail_bwd",
        )
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


def gpt_block_head(x, ln1, q, kv, pair=None):
    """pair: a dict shared with gpt_block_tail of the SAME block (one per forward): lets the two backward
    kernels share one weight-gradient reduction launch. pair["chain"] = ops.new_block_chain() shared by ALL blocks of a model and
    pair["flush"] = True on the block whose backward runs last (the model's first block): one reduction launch per 8 blocks."""
    params = (ln1.weight, ln1.bias, q.weight, q.bias, kv.weight, kv.bias)
    return _GPTBlockHead.apply(x, *params, float(ln1.eps), params, pair)


def gpt_block_tail(o, x, proj, ln2, fc1, fc2, pair=None, next_head=None):
    """next_head = (ln1, q, kv) of the FOLLOWING block (which must pass gpt_block_supported too): its LN1 and q/kv projection run
    in this block's tail launch, and the qkv waits in pair["boundary"] — a dict shared by the blocks of one forward — for the
    gpt_block_head call of that block on the tensor returned here."""
    params = (proj.weight, proj.bias, ln2.weight, ln2.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias)
    eps = float(ln2.eps)
    if next_head is not None and pair is not None and pair.get("boundary") is not None:
        ln1, q, kv = next_head
        if float(ln1.eps) == eps:  # one eps serves both LayerNorms of the launch
            pair["next_head"] = (ln1.weight, ln1.bias, q.weight, q.bias, kv.weight, kv.bias)
    return _GPTBlockTail.apply(o, x, *params, eps, params, pair)


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
