"""ops.conv — convolution over a tap list (forward, data / weight gradient, fused epilogues, pass-through aliases).

Part of the operator layer (pytorch_generative_amd.ops): HIP kernels behind torch.autograd.Function, called through the C-ABI
with tensor.data_ptr() and the current stream. No CPU / ATen fallback: a missing library, a CPU tensor or an unsupported shape raises."""

import os
from typing import NamedTuple, Optional

import torch

from pytorch_generative_amd import _lib
from pytorch_generative_amd.ops._common import (
    ACT_ELU,
    ACT_ELU_OUT,
    ACT_NONE,
    ACT_RELU,
    CONV_FMT_B3,
    CONV_FMT_B3_GATE,
    FUSE_SKIP,
    _chk,
    _dense_per_image,
    _grad_targets,
    _p,
    _sink,
    _stream,
)
from pytorch_generative_amd.ops.elementwise import add


# --------------------------------------------------------------------------------------------
# convolution over a tap list
# --------------------------------------------------------------------------------------------
class ConvSpec:
    """Static description of one stride-1 convolution as tap lists.

    out[r, c] = sum_t w[:, :, u_t, v_t] . x[r + u_t - pad_h, c + v_t - pad_w]
    `active` restricts the forward/data-grad taps (the causal mask's non-zero entries,
    reference nn/convolution.py:35-39). The weight gradient always covers `wgrad_taps`
    (all taps by default: the reference's weight.grad is unmasked, nn/convolution.py:42).
    """

    def __init__(self, kh, kw, pad_h, pad_w, active=None, wgrad_all=True):
        self.kh, self.kw, self.pad_h, self.pad_w = kh, kw, pad_h, pad_w
        all_taps = [(u, v) for u in range(kh) for v in range(kw)]
        act = all_taps if active is None else [t for t in all_taps if t in set(active)]
        if not act:
            raise ValueError("ConvSpec: no active taps")
        if len(all_taps) > 64:
            raise ValueError(f"ConvSpec: {kh}x{kw} kernel has more than 64 taps")
        self.fwd_taps = act
        self.wg_taps = all_taps if wgrad_all else act
        ia = _lib.int_array
        self.f_dr = ia([u - pad_h for u, _ in act])
        self.f_dc = ia([v - pad_w for _, v in act])
        self.f_ndr = ia([pad_h - u for u, _ in act])
        self.f_ndc = ia([pad_w - v for _, v in act])
        self.f_u = ia([u for u, _ in act])
        self.f_v = ia([v for _, v in act])
        self.w_dr = ia([u - pad_h for u, _ in self.wg_taps])
        self.w_dc = ia([v - pad_w for _, v in self.wg_taps])
        self.w_u = ia([u for u, _ in self.wg_taps])
        self.w_v = ia([v for _, v in self.wg_taps])
        # extent of the active tap list (identical for the negated list of the data gradient)
        self.hr = max(u for u, _ in act) - min(u for u, _ in act)
        self.hc = max(v for _, v in act) - min(v for _, v in act)
        self._fmts = {}  # _use_mfma's answers for this tap list

    def full_out(self, h, w):
        return h + 2 * self.pad_h - self.kh + 1, w + 2 * self.pad_w - self.kw + 1


# A/B switches for measurements: PG_CONV_MFMA=0 keeps every convolution on the VALU tap kernels, PG_FUSE_PAIR=0 /
# PG_FUSE_LNSKIP=0 select the unfused graphs
CONV_MFMA = os.environ.get("PG_CONV_MFMA", "1") != "0"
FUSE_PAIR = os.environ.get("PG_FUSE_PAIR", "1") != "0"
FUSE_LNSKIP = os.environ.get("PG_FUSE_LNSKIP", "1") != "0"
FUSE_QKV_EXTRA = os.environ.get("PG_FUSE_QKV_EXTRA", "1") != "0"  # CausalAttention with extra_x: merged [q|k|v] projection
FUSE_DUAL = os.environ.get("PG_FUSE_DUAL", "1") != "0"  # 0 = pg_act_bwd_from_out launches behind the block tail's convolutions
FUSE_GATE = os.environ.get("PG_FUSE_GATE", "1") != "0"  # 0 = the standalone gate kernel behind the convolution


def _use_mfma(lib, k_channels, m_channels, spec, out_hw, in_w):
    """Fragment format of the matrix-core path for this problem (0: none -> VALU tap kernels,
    1: fp32 MFMA, 2: bf16x3 MFMA; include/pg_hip.h PG_CONV_FMT_*). The library's answer is a host function of these
    integers and the tap list for the life of the process: asked once per ConvSpec and problem."""
    if not CONV_MFMA:
        return 0
    key = (int(k_channels), int(m_channels), int(out_hw[0]), int(out_hw[1]), int(in_w))
    fmt = spec._fmts.get(key)
    if fmt is None:
        fmt = spec._fmts[key] = int(lib.pg_conv_mfma_supported(*key[:2], len(spec.fwd_taps), *key[2:], spec.hr, spec.hc))
    return fmt


def conv_formats(wshape, spec, in_hw, out_hw=None, fwd=True, dgrad=True):
    """(forward, data-gradient) fragment formats for an in_hw input, a wshape weight and out_hw (default: the full extent);
    an orientation not asked for is 0. The data gradient is the same convolution with channels and extents exchanged."""
    cout, cin = wshape[0], wshape[1]
    out_hw = spec.full_out(*in_hw) if out_hw is None else out_hw
    lib = _lib.load()
    return (_use_mfma(lib, cin, cout, spec, out_hw, in_hw[1]) if fwd else 0,
            _use_mfma(lib, cout, cin, spec, in_hw, out_hw[1]) if dgrad else 0)


def _pack_frag(lib, weight, spec, transpose, fmt):
    """MFMA A-fragment pack of the active taps (csrc/conv_mfma.hip, csrc/conv_b3.hip)."""
    cout, cin, kh, kw = weight.shape
    kc, m = (cout, cin) if transpose else (cin, cout)
    t = len(spec.fwd_taps)
    wfrag = torch.empty(lib.pg_conv_frag_floats(kc, m, t, fmt), device=weight.device, dtype=torch.float32)
    _lib.check(
        lib.pg_pack_conv_weight_frag(weight.data_ptr(), wfrag.data_ptr(), cout, cin, kh, kw, t,
                                     spec.f_u, spec.f_v, int(transpose), fmt, _stream()),
        "pg_pack_conv_weight_frag",
    )
    return wfrag


def _pack_frags(lib, weight, spec, fmt_f, fmt_t):
    """(forward fragments, data-gradient fragments or None): one orientation, or both from one launch when the data
    gradient has a format too (fmt_t != 0: backward then packs nothing)."""
    if not fmt_t:
        return _pack_frag(lib, weight, spec, False, fmt_f), None
    cout, cin, kh, kw = weight.shape
    t = len(spec.fwd_taps)
    wf = torch.empty(lib.pg_conv_frag_floats(cin, cout, t, fmt_f), device=weight.device, dtype=torch.float32)
    wt = torch.empty(lib.pg_conv_frag_floats(cout, cin, t, fmt_t), device=weight.device, dtype=torch.float32)
    _lib.check(
        lib.pg_pack_conv_weight_frag2(weight.data_ptr(), wf.data_ptr(), wt.data_ptr(), cout, cin, kh,
                                      kw, t, spec.f_u, spec.f_v, fmt_f, fmt_t, _stream()),
        "pg_pack_conv_weight_frag2",
    )
    return wf, wt


def _pack(lib, weight, spec, transpose):
    cout, cin, kh, kw = weight.shape
    a, b = (cout, cin) if transpose else (cin, cout)
    t = len(spec.fwd_taps)
    b_pad = lib.pg_conv_b_pad(b)
    wpk = torch.empty(a * t * b_pad, device=weight.device, dtype=torch.float32)
    _lib.check(
        lib.pg_pack_conv_weight(
            weight.data_ptr(), wpk.data_ptr(), cout, cin, kh, kw, t, spec.f_u, spec.f_v,
            int(transpose), b_pad, _stream(),
        ),
        "pg_pack_conv_weight",
    )
    return wpk


class GradSlot:
    """One gradient tensor handed from a consumer's backward to a producer's backward outside autograd's own edges: the "dual"
    data gradient (conv2d_taps(..., in_sum=(r, slot))) computes TWO gradients for its one input x = elu(a) + r — autograd carries
    the first (a's), the second (r's, already multiplied by r's ELU derivative) waits here for the backward of the convolution that
    added r (conv2d_taps(..., out_pre_scaled=True, res=r, res_slot=slot)), which returns it as r's gradient. Filled and emptied
    once per backward pass; taking from an empty slot raises (the consumer's backward did not run first, or took another path)."""

    def __init__(self):
        self._g = None

    def put(self, g):
        if self._g is not None:
            raise RuntimeError("GradSlot: filled twice in one backward pass")
        self._g = g

    def take(self):
        g, self._g = self._g, None
        if g is None:
            raise RuntimeError("GradSlot: empty — the dual data gradient that fills it has not run")
        return g


class _Call(NamedTuple):
    """Everything about one convolution call that is not a tensor, resolved once outside autograd (_resolve) and read by
    the protocol check, the forward and the backward."""

    spec: ConvSpec
    in_hw: tuple
    out_hw: tuple
    fmt: int  # forward fragment format (0: VALU tap kernel)
    fmt_t: int  # the data gradient's; asked only when x needs a gradient
    need_dx: bool
    in_act: int = ACT_NONE
    out_act: int = ACT_NONE
    out_pre_scaled: bool = False
    in_post: int = ACT_NONE
    n_skip: int = 0  # pass-through aliases of x whose gradients come back to this node
    gate: Optional[int] = None
    has_bias: bool = False
    has_res: bool = False
    has_res2: bool = False
    has_gate_res: bool = False
    has_in_sum: bool = False
    gw: Optional[torch.Tensor] = None  # gradient sinks of weight / bias (None: the gradient goes to autograd)
    gb: Optional[torch.Tensor] = None
    res_slot: Optional[GradSlot] = None  # where backward takes res's gradient from / puts the second input gradient
    in_sum_slot: Optional[GradSlot] = None


def _resolve(wshape, spec, in_hw, out_hw, need_dx, **options):
    in_hw, out_hw = tuple(map(int, in_hw)), tuple(map(int, out_hw))
    fmt, fmt_t = conv_formats(wshape, spec, in_hw, out_hw, dgrad=need_dx)
    return _Call(spec, in_hw, out_hw, fmt, fmt_t, bool(need_dx), **options)


def _check_call(call, wshape, xshape, res=None, res2=None, gate_res=None, in_sum=None):
    """Every protocol refusal of the convolution, raised before anything is launched. `res` .. `in_sum` are the SHAPES of
    the optional operands; no tensor is looked at (the format and dual queries are host functions of the library)."""
    n, cin = xshape[0], xshape[1]
    cout = wshape[0]
    out_shape = (n, cout) + call.out_hw
    act_out = call.out_act != ACT_NONE
    if wshape[1] != cin:
        raise ValueError(f"conv2d: weight expects {wshape[1]} input channels, got {cin}")
    if call.has_res and tuple(res) != out_shape:
        raise ValueError("conv2d: residual shape mismatch")
    if call.has_res2:
        if not call.has_res or tuple(res2) != out_shape:
            raise ValueError("conv2d: res2 needs res and the output's shape")
        if not (call.fmt == CONV_FMT_B3 and cout >= 64):
            raise ValueError("conv2d: a second residual needs the bf16x3 kernel with >= 64 output channels "
                             "(check ops.conv_two_residuals_ok first)")
    if call.out_pre_scaled and call.has_res and call.res_slot is not None:
        # the consumer is a dual data gradient (in_sum): it recovers this activation's output as (its input - res) and hands
        # res's gradient back through the slot
        if call.out_act != ACT_ELU or call.has_res2:
            raise ValueError("conv2d: res_slot needs out_act='elu' and a single residual")
    elif call.out_pre_scaled and call.has_res:
        # the consumer (in_post) recovers act' from THIS output: a residual added behind the activation would change
        # the value it reads and with it every gradient upstream (found by tests/test_gpu_ops.py::test_conv_protocol_matrix)
        raise ValueError("conv2d: out_pre_scaled cannot be combined with a residual (the consumer's in_post derivative "
                         "is taken from this convolution's output)")
    if call.out_pre_scaled and not act_out:
        raise ValueError("conv2d: out_pre_scaled without an output activation")
    if (act_out or call.in_post != ACT_NONE) and not call.fmt:
        raise ValueError("conv2d: fused output activations need the matrix-core path "
                         "(check ops.conv_mfma_ok first)")
    if call.gate is not None:
        if call.fmt != CONV_FMT_B3 or call.has_res2 or act_out:
            raise ValueError("conv2d: gate= needs a bf16x3 convolution with at most one residual (check ops.conv_gate_ok first)")
        if call.has_gate_res and tuple(gate_res) != (n, cout // 2) + call.out_hw:
            raise ValueError("conv2d: gate_res shape mismatch")
    if call.has_in_sum:
        if call.gate is not None or call.n_skip or call.in_act != ACT_ELU or tuple(in_sum) != tuple(xshape):
            raise ValueError("conv2d: in_sum needs in_act='elu', no skip aliases and r of the input's shape")
        if not _dual_ok(wshape, call.spec, call.in_hw):
            raise ValueError("conv2d: in_sum on a shape the dual data gradient does not take (check ops.conv_dual_ok first)")
    # the producer of x skipped its activation derivative on the promise that THIS data gradient's
    # epilogue applies it (out_pre_scaled / in_post protocol): only the matrix-core epilogue can
    if call.in_post != ACT_NONE and call.in_act != ACT_NONE:
        raise ValueError("conv2d: in_act and in_post cannot both be set (one epilogue derivative)")
    if call.in_post != ACT_NONE and call.need_dx and not call.fmt_t:
        raise RuntimeError("conv2d: in_post needs the matrix-core data gradient (shape not covered): "
                           "the activation derivative of the producer would be dropped")


def _conv_forward(ctx, call, x, weight, bias, res=None, res2=None, gate_res=None, r_sum=None):
    """The forward of a checked call: y (the gated half where call.gate is set), then the skip aliases of x."""
    lib = _lib.load()
    spec, gated = call.spec, call.gate is not None
    x = _chk(x, "conv2d.x")
    weight = _chk(weight, "conv2d.weight")
    bias = bias if bias is None else _chk(bias, "conv2d.bias")
    res = res if res is None else _chk(res, "conv2d.res")
    if res2 is not None and not _dense_per_image(res2):
        res2 = _chk(res2, "conv2d.res2")  # (a channel slice of a wider tensor is read with its batch stride, no copy)
    gate_res = gate_res if gate_res is None else _chk(gate_res, "conv2d.gate_res")
    r_sum = r_sum if r_sum is None else _chk(r_sum, "conv2d.in_sum")
    n, cin, ih, iw = x.shape
    cout, (oh, ow), taps = weight.shape[0], call.out_hw, len(spec.fwd_taps)
    out = y = torch.empty((n, cout, oh, ow), device=x.device, dtype=torch.float32)
    wfrag_t = None
    if call.fmt:
        # (gate: forward fragments in the gate-interleaved channel order, each wave owns both halves of its gate channels)
        wfrag, wfrag_t = _pack_frags(lib, weight, spec, CONV_FMT_B3_GATE if gated else call.fmt, call.fmt_t)
    if gated:
        # GatedActivation (+ the residual behind it) in the convolution's epilogue: `out` keeps the pre-gate values for
        # backward (the convolution's own residual is part of them; its gradient is the gate's input gradient), y is what
        # the caller sees
        y = torch.empty((n, cout // 2, oh, ow), device=x.device, dtype=torch.float32)
        _lib.check(
            lib.pg_conv2d_mfma_gate(
                x.data_ptr(), wfrag.data_ptr(), _p(bias), _p(res), out.data_ptr(), n, cin, ih, iw, cout, oh, ow,
                taps, spec.f_dr, spec.f_dc, call.in_act, call.gate, _p(gate_res), y.data_ptr(), _stream(),
            ),
            "pg_conv2d_mfma_gate",
        )
    elif call.fmt:
        _lib.check(
            lib.pg_conv2d_mfma_ex(
                x.data_ptr(), wfrag.data_ptr(), _p(bias), _p(res), out.data_ptr(), n, cin, ih,
                iw, cout, oh, ow, taps, spec.f_dr, spec.f_dc, call.in_act, 0, ACT_NONE,
                call.out_act, call.fmt, _p(res2), 0, res2.stride(0) if res2 is not None else 0, _stream(),
            ),
            "pg_conv2d_mfma",
        )
    else:
        wpk = _pack(lib, weight, spec, transpose=False)
        _lib.check(
            lib.pg_conv2d_taps(
                x.data_ptr(), wpk.data_ptr(), _p(bias), _p(res), out.data_ptr(), n, cin, ih, iw,
                cout, oh, ow, taps, spec.f_dr, spec.f_dc, call.in_act, 0, ACT_NONE, _stream(),
            ),
            "pg_conv2d_taps",
        )
    # an unscaled output activation: backward recovers act' from the output, v = out - res
    from_out = call.out_act != ACT_NONE and not call.out_pre_scaled
    ctx.call, ctx.wfrag_t = call, wfrag_t
    ctx.save_for_backward(x, weight, out if gated or from_out else None, res if from_out else None, r_sum)
    # pass-through aliases of x for skip connections: their consumers' gradients come back to THIS
    # node's backward and are added in the data gradient's epilogue (no gradient-sum kernel)
    return (y,) + tuple(x.view_as(x) for _ in range(call.n_skip)) if call.n_skip else y


def _gate_grad(lib, z, dy, gate):
    """dz (both halves) from the stored pre-gate output z and the gradient of the gated half."""
    nz, c2, hz, wz = z.shape
    dz = torch.empty_like(z)
    _lib.check(lib.pg_gated_bwd(z.data_ptr(), dy.data_ptr(), dz.data_ptr(), nz, c2 // 2, hz * wz, gate, _stream()),
               "pg_gated_bwd")
    return dz


def _data_grad(lib, call, x, wpk_t, dy, r_sum, skips):
    """dx (through a fused input activation) plus the gradients `skips` of x's aliases; wpk_t: weights packed for call.fmt_t."""
    spec = call.spec
    n, cin, ih, iw = x.shape
    _, cout, oh, ow = dy.shape
    taps, n_fused = len(spec.fwd_taps), 0
    dx = torch.empty_like(x)
    if call.fmt_t:
        # matrix-core data gradient; act'(x) of a fused input activation in its epilogue (one
        # exp / erf per output element is noise next to the MFMA work of the tile)
        dact = call.in_act if call.in_act != ACT_NONE else (ACT_ELU_OUT if call.in_post == ACT_ELU else ACT_NONE)
        if call.in_sum_slot is not None:
            # dual: dx = the gradient of a's pre-activation (x = elu(a) + r), the second output that of r's producer
            dx2 = torch.empty_like(x)
            _lib.check(lib.pg_conv2d_mfma_dual(dy.data_ptr(), wpk_t.data_ptr(), dx.data_ptr(), dx2.data_ptr(), n, cout, oh, ow,
                                               cin, x.data_ptr(), dact, r_sum.data_ptr(), _stream()), "pg_conv2d_mfma_dual")
            call.in_sum_slot.put(dx2)
        else:
            # up to two skip gradients ride in the epilogue of the bf16x3 kernel (dx = dgrad * act' + skip1 + skip2; the
            # multi-stream epilogue exists for >= 64 output channels); a skip may be a channel slice of a wider gradient
            # (batch-strided)
            n_fused = min(len(skips), 2) if call.fmt_t == CONV_FMT_B3 and cin >= 64 else 0
            for i in range(n_fused):
                if not _dense_per_image(skips[i]):
                    skips[i] = _chk(skips[i], "conv2d.d_skip")  # (in the caller's list: the copy lives as long as dx)
            r1, r2 = (skips[:n_fused] + [None, None])[:2]
            _lib.check(
                lib.pg_conv2d_mfma_ex(
                    dy.data_ptr(), wpk_t.data_ptr(), 0, _p(r1), dx.data_ptr(), n, cout, oh, ow, cin,
                    ih, iw, taps, spec.f_ndr, spec.f_ndc, ACT_NONE,
                    x.data_ptr() if dact != ACT_NONE else 0, dact, ACT_NONE, call.fmt_t, _p(r2),
                    r1.stride(0) if r1 is not None else 0, r2.stride(0) if r2 is not None else 0, _stream(),
                ),
                "pg_conv2d_mfma(dgrad)",
            )
    else:
        # ReLU's derivative is applied in the dgrad kernel's epilogue; for ELU/GELU (exp/erf:
        # ~40 instructions per element) the fused epilogue measured SLOWER than a separate
        # streaming pass (107 us vs 25 + 47 us on the ImageGPT MLP), so they stay separate.
        fuse = call.in_act == ACT_RELU
        _lib.check(
            lib.pg_conv2d_taps(
                dy.data_ptr(), wpk_t.data_ptr(), 0, 0, dx.data_ptr(), n, cout, oh, ow, cin, ih,
                iw, taps, spec.f_ndr, spec.f_ndc, ACT_NONE,
                x.data_ptr() if fuse else 0, call.in_act if fuse else ACT_NONE, _stream(),
            ),
            "pg_conv2d_taps(dgrad)",
        )
        if call.in_act != ACT_NONE and not fuse:
            _lib.check(
                lib.pg_act_bwd(x.data_ptr(), dx.data_ptr(), dx.data_ptr(), dx.numel(), call.in_act, _stream()),
                "pg_act_bwd",
            )
    for g in skips[n_fused:]:  # the VALU kernel, another format than bf16x3, or more than two
        dx = add(dx, _chk(g, "conv2d.d_skip"))
    return dx


def _weight_grad(lib, call, x, weight, need_b, dy):
    """Adds the weight (and, with need_b, the bias) gradient into the sinks or fresh tensors: (dw, db) for autograd."""
    spec = call.spec
    n, cin, ih, iw = x.shape
    _, cout, oh, ow = dy.shape
    # (a bias is not saved for its shape: a merged bias computed in forward would live until here; one entry per output channel)
    tgt, ret = _grad_targets([weight, weight[:, 0, 0, 0]] if need_b else [weight], (call.gw, call.gb))
    gw_t, gb_t = tgt + [None] * (not need_b)
    ws_n = lib.pg_conv2d_wgrad_workspace_floats(cout, cin, len(spec.wg_taps))
    ws = torch.empty(ws_n, device=x.device, dtype=torch.float32)
    _lib.check(
        lib.pg_conv2d_wgrad(
            x.data_ptr(), dy.data_ptr(), gw_t.data_ptr(), _p(gb_t), n, cin, ih, iw, cout,
            oh, ow, spec.kh, spec.kw, len(spec.wg_taps), spec.w_dr, spec.w_dc, spec.w_u,
            spec.w_v, call.in_act, ws.data_ptr(), ws_n, _stream(),
        ),
        "pg_conv2d_wgrad",
    )
    return tuple(ret + [None] * (not need_b))


def _conv_backward(ctx, dy, need_w, need_b, d_skips=()):
    """(dx, dw, db, dres, dres2, dgate_res) of a _conv_forward under the same ctx."""
    lib = _lib.load()
    call = ctx.call
    x, weight, out, res, r_sum = ctx.saved_tensors
    dy = _chk(dy, "conv2d.dy")
    dres2 = dy if call.has_res2 else None
    dgate_res = dy if call.gate is not None and call.has_gate_res else None
    if call.gate is not None:
        dy = _gate_grad(lib, out, dy, call.gate)  # through the gate first, then the usual data / weight gradients
    dres = dy if call.has_res else None
    if call.has_res and call.res_slot is not None:
        dres = call.res_slot.take()  # the residual's gradient, already through ITS producer's ELU (dual data gradient)
    if call.out_act != ACT_NONE and not call.out_pre_scaled:
        g = torch.empty_like(dy)
        _lib.check(lib.pg_act_bwd_from_out(out.data_ptr(), _p(res), dy.data_ptr(), g.data_ptr(),
                                           dy.numel(), call.out_act, _stream()), "pg_act_bwd_from_out")
        dy = g
    skips = [g for g in d_skips if g is not None]
    dx = wpk_t = None
    if call.need_dx:
        # (packed here: like every buffer of this backward it lives to the end, the allocator's reuse pattern depends on it)
        wpk_t = ctx.wfrag_t
        if wpk_t is None:
            wpk_t = _pack_frag(lib, weight, call.spec, True, call.fmt_t) if call.fmt_t else _pack(lib, weight, call.spec, True)
        dx = _data_grad(lib, call, x, wpk_t, dy, r_sum, skips)
    dw, db = _weight_grad(lib, call, x, weight, need_b, dy) if need_w or need_b else (None, None)
    if skips and not call.need_dx:
        raise RuntimeError("conv2d: skip outputs of an input that needs no gradient received gradients")
    return dx, dw, db, dres, dres2, dgate_res


class _ConvTaps(torch.autograd.Function):
    @staticmethod
    def forward(ctx, call, x, weight, bias, res, res2, gate_res, r_sum):
        return _conv_forward(ctx, call, x, weight, bias, res, res2, gate_res, r_sum)

    @staticmethod
    def backward(ctx, dy, *d_skips):
        need = ctx.needs_input_grad
        return (None,) + _conv_backward(ctx, dy, need[2], ctx.call.has_bias and need[3], d_skips) + (None,)


def _adjacent_view(a, b, shape):
    """One tensor over `a` followed immediately by `b` in the same storage (None if they are not
    laid out that way): FlatAdam places declared pairs back to back (optim.py, `_pg_follows`)."""
    if a is None or b is None or a.dtype != torch.float32 or b.dtype != torch.float32:
        return None
    if not (a.is_contiguous() and b.is_contiguous()) or a.device != b.device:
        return None
    if a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr():
        return None
    if a.data_ptr() + 4 * a.numel() != b.data_ptr():
        return None
    strides, acc = [], 1
    for d in reversed(shape):
        strides.append(acc)
        acc *= d
    return a.as_strided(tuple(shape), tuple(reversed(strides)), a.storage_offset())


def conv_pair_views(conv_a, conv_b):
    """(weight, bias, weight-grad sink, bias-grad sink) of the concatenated convolution
    [conv_a; conv_b] as zero-copy views, or None when the two modules' parameters / gradient sinks
    are not adjacent in the flat buffers (then the caller runs the two convolutions separately)."""
    wa, wb = conv_a.weight, conv_b.weight
    if conv_a.bias is None or conv_b.bias is None or wa.shape[1:] != wb.shape[1:]:
        return None
    ca, cb = wa.shape[0], wb.shape[0]
    wshape = (ca + cb,) + tuple(wa.shape[1:])
    w = _adjacent_view(wa.data, wb.data, wshape)
    b = _adjacent_view(conv_a.bias.data, conv_b.bias.data, (ca + cb,))
    gw = _adjacent_view(_sink(wa), _sink(wb), wshape)
    gb = _adjacent_view(_sink(conv_a.bias), _sink(conv_b.bias), (ca + cb,))
    if w is None or b is None or gw is None or gb is None:
        return None
    return w, b, gw, gb


class _ConvPair(torch.autograd.Function):
    """y = [conv_a(x); conv_b(x)] (channel concatenation) as ONE tap convolution over the merged
    parameter views: x is read once, one data gradient (no autograd accumulation pass over dx), one
    weight-gradient launch writing straight into the merged gradient sinks."""

    @staticmethod
    def forward(ctx, call, x, wa, ba, wb, bb, w, b):
        return _conv_forward(ctx, call, x, w, b)

    @staticmethod
    def backward(ctx, dy):
        need = ctx.needs_input_grad
        dx = _conv_backward(ctx, dy, need[2] or need[4], need[3] or need[5])[0]
        return None, dx, None, None, None, None, None, None


def conv2d_pair(x, conv_a, conv_b, views, spec, out_hw=None):
    if out_hw is None:
        out_hw = spec.full_out(x.shape[2], x.shape[3])
    w, b, gw, gb = views
    call = _resolve(w.shape, spec, x.shape[2:], out_hw, x.requires_grad, has_bias=True, gw=gw, gb=gb)
    _check_call(call, w.shape, x.shape)
    return _ConvPair.apply(call, x, conv_a.weight, conv_a.bias, conv_b.weight, conv_b.bias, w, b)


def conv2d_taps(x, weight, bias, spec, out_hw=None, in_act=ACT_NONE, res=None,
                weight_param=None, bias_param=None, out_act=ACT_NONE, out_pre_scaled=False,
                in_post=ACT_NONE, n_skip=0, res2=None, gate=None, gate_res=None, res_slot=None, in_sum=None):
    """y = out_act(conv(in_act(x)) + bias) (+ res), cropped to out_hw (defaults to the full extent).

    out_act (matrix-core path only): activation fused into the epilogue; its backward recovers act'
    from the output (ELU / ReLU). out_pre_scaled=True declares that the ONLY consumer of y hands back
    a gradient already multiplied by act'(y) — the consumer is a convolution called with
    in_post=<that activation>, which applies the factor in its data-gradient epilogue.

    n_skip > 0 returns (y, x_1, ..., x_n): pass-through aliases of x for the skip connections that also
    read x (residual adds, later concatenations). Using them instead of x makes this op x's ONLY consumer,
    so autograd never sums gradients for x: the skip gradients arrive in this op's backward and are added
    in the data-gradient kernel's epilogue. A combination the kernels cannot take raises here (_check_call)."""
    full = spec.full_out(x.shape[2], x.shape[3])
    if out_hw is None:
        out_hw = full
    # outputs beyond the "full" extent read only zero padding; allow up to one kernel's worth
    # (used by the phase-decomposed stride-2 convolutions)
    if out_hw[0] > full[0] + spec.kh or out_hw[1] > full[1] + spec.kw or min(out_hw) < 1:
        raise ValueError(f"conv2d: requested output {out_hw} exceeds the full extent {full}")
    r_sum, in_sum_slot = in_sum if in_sum is not None else (None, None)
    call = _resolve(
        weight.shape, spec, x.shape[2:], out_hw, x.requires_grad, in_act=in_act, out_act=out_act,
        out_pre_scaled=bool(out_pre_scaled), in_post=in_post, n_skip=int(n_skip) if FUSE_SKIP else 0, gate=gate,
        has_bias=bias is not None, has_res=res is not None, has_res2=res2 is not None, has_gate_res=gate_res is not None,
        has_in_sum=in_sum is not None, gw=_sink(weight_param), gb=_sink(bias_param), res_slot=res_slot,
        in_sum_slot=in_sum_slot)
    _check_call(call, weight.shape, x.shape, *(t if t is None else t.shape for t in (res, res2, gate_res, r_sum)))
    # (r reaches this node's backward as a saved value and leaves it through the slot: no autograd edge to its producer)
    y = _ConvTaps.apply(call, x, weight, bias, res, res2, gate_res, r_sum if r_sum is None else r_sum.detach())
    if n_skip and not FUSE_SKIP:
        return (y,) + (x,) * int(n_skip)
    return y


def conv_mfma_ok(x, weight, spec, out_hw=None):
    """True if this convolution AND its data gradient run on the matrix-core kernels (the fused
    output-activation / post-activation-input protocols of conv2d_taps need both)."""
    return bool(x.is_cuda and all(conv_formats(weight.shape, spec, x.shape[2:], out_hw)))


def conv_two_residuals_ok(x, weight, spec, out_hw=None):
    """True if conv2d_taps(..., res=, res2=) is available for this problem (bf16x3 kernel, >= 64 output channels)."""
    return bool(x.is_cuda and weight.shape[0] >= 64
                and conv_formats(weight.shape, spec, x.shape[2:], out_hw, dgrad=False)[0] == CONV_FMT_B3)


def _dual_ok(wshape, spec, in_hw):
    if not FUSE_DUAL or tuple(wshape[2:]) != (1, 1) or len(spec.fwd_taps) != 1 or spec.f_dr[0] != 0 or spec.f_dc[0] != 0:
        return False
    if conv_formats(wshape, spec, in_hw, in_hw, fwd=False)[1] != CONV_FMT_B3:
        return False
    return bool(_lib.load().pg_conv_dual_ok(int(wshape[0]), int(wshape[1]), int(in_hw[0]), int(in_hw[1])))


def conv_dual_ok(x, weight, spec):
    """True if conv2d_taps(x, ..., in_act=elu, in_sum=(r, slot)) can deliver both producers' gradients from its data
    gradient's epilogue (pg_conv_dual_ok: a 1x1 convolution whose data gradient runs on the bf16x3 1x1 kernel)."""
    return bool(x.is_cuda and x.dtype == torch.float32 and _dual_ok(weight.shape, spec, x.shape[2:]))


def conv_gate_ok(x, weight, spec, out_hw=None):
    """True if conv2d_taps(..., gate=...) can fuse the GatedActivation that follows this convolution into its launch
    (pg_conv_gate_fusable: bf16x3 format on the wide kernel, a multiple of 128 output channels)."""
    if not FUSE_GATE or not x.is_cuda or x.dtype != torch.float32:
        return False
    oh, ow = out_hw if out_hw is not None else spec.full_out(x.shape[2], x.shape[3])
    if conv_formats(weight.shape, spec, x.shape[2:], (oh, ow), dgrad=False)[0] != CONV_FMT_B3:
        return False
    return bool(_lib.load().pg_conv_gate_fusable(int(weight.shape[1]), int(weight.shape[0]), oh, ow, len(spec.fwd_taps),
                                                 spec.f_dr, spec.f_dc))
