"""CPU: the Python glue every convolution passes through — ops.conv's call record, its one protocol check and the memoised
format query, and nn.Conv2d.forward's choice of what the kernels fuse — without a GPU. The library's host-only queries
(pg_conv_mfma_supported, pg_conv_gate_fusable, pg_conv_dual_ok) run here; nothing is launched."""

import itertools
import random

import pytest
import torch

from pytorch_generative_amd import nn as pg_nn
from pytorch_generative_amd import ops
from pytorch_generative_amd.ops import conv as opconv
from test_gpu_ops import PROTOCOL_SHAPES

ELU, RELU = ops.ACT_ELU, ops.ACT_RELU
S1, S2, S3 = ops.ConvSpec(1, 1, 0, 0), ops.ConvSpec(2, 2, 1, 1), ops.ConvSpec(3, 3, 1, 1)
# (weight shape, spec, input extent, output extent) and what the format query says about each (asserted below)
B3 = ((64, 64, 3, 3), S3, (16, 16), (16, 16))      # bf16x3 both ways, >= 64 output channels
GATE = ((128, 64, 2, 2), S2, (16, 16), (16, 16))   # bf16x3 on the wide kernel: the gate fuses (PixelSNAIL's cropped 2x2)
DUAL = ((64, 64, 1, 1), S1, (16, 16), (16, 16))    # 1x1 whose data gradient runs on the bf16x3 1x1 kernel
F32 = ((32, 32, 3, 3), S3, (8, 8), (8, 8))         # matrix cores, fewer than 64 output channels
NO_DGRAD = ((32, 3, 3, 3), S3, (12, 12), (12, 12))  # fp32-MFMA forward, no matrix-core data gradient (3 output channels)
VALU = ((16, 3, 3, 3), S3, (12, 12), (12, 12))     # VALU tap kernels both ways
N = 2


def test_the_shapes_of_this_file_route_as_labelled(lib):
    fmts = {name: ops.conv_formats(*p) for name, p in (("B3", B3), ("GATE", GATE), ("DUAL", DUAL), ("F32", F32),
                                                       ("NO_DGRAD", NO_DGRAD), ("VALU", VALU))}
    assert fmts["B3"] == fmts["GATE"] == fmts["DUAL"] == (ops.CONV_FMT_B3, ops.CONV_FMT_B3), fmts
    assert all(fmts["F32"]) and fmts["NO_DGRAD"][0] and not fmts["NO_DGRAD"][1] and fmts["VALU"] == (0, 0), fmts
    (cout, cin, _, _), spec, _, (oh, ow) = GATE
    assert lib.pg_conv_gate_fusable(cin, cout, oh, ow, len(spec.fwd_taps), spec.f_dr, spec.f_dc)
    assert opconv._dual_ok(*DUAL[:3]) and not opconv._dual_ok(*B3[:3])


def _check(problem, need_dx=True, cin=None, res=None, res2=None, gate_res=None, in_sum=None, **options):
    """The protocol check of one call on `problem`: `res` .. `in_sum` are True (an operand of the right shape) or a shape."""
    wshape, spec, in_hw, out_hw = problem
    xshape = (N, wshape[1] if cin is None else cin) + in_hw
    right = {"res": (N, wshape[0]) + out_hw, "res2": (N, wshape[0]) + out_hw, "gate_res": (N, wshape[0] // 2) + out_hw,
             "in_sum": xshape}
    given = {"res": res, "res2": res2, "gate_res": gate_res, "in_sum": in_sum}
    shapes = {k: (right[k] if v is True else v) for k, v in given.items()}
    call = opconv._resolve(wshape, spec, in_hw, out_hw, need_dx, **{f"has_{k}": v is not None for k, v in shapes.items()},
                           **options)
    opconv._check_call(call, wshape, xshape, **shapes)
    return call


SLOT = ops.GradSlot()
# (what, exception, fragment of its message, the smallest refused call, the nearest allowed call): one line per refusal of
# the convolution's protocol; each call is (problem, keyword arguments of _check)
REFUSALS = [
    ("weight / input channels", ValueError, "input channels", (B3, dict(cin=32)), (B3, dict())),
    ("res of another shape", ValueError, "residual shape mismatch", (B3, dict(res=(N, 64, 16, 15))), (B3, dict(res=True))),
    ("res2 without res", ValueError, "res2 needs res", (B3, dict(res2=True)), (B3, dict(res=True, res2=True))),
    ("res2 of another shape", ValueError, "res2 needs res", (B3, dict(res=True, res2=(N, 32, 16, 16))),
     (B3, dict(res=True, res2=True))),
    ("res2 under 64 output channels", ValueError, "second residual needs the bf16x3 kernel", (F32, dict(res=True, res2=True)),
     (B3, dict(res=True, res2=True))),
    ("res2 on the VALU kernel", ValueError, "second residual needs the bf16x3 kernel", (VALU, dict(res=True, res2=True)),
     (VALU, dict(res=True))),
    ("res_slot behind another activation", ValueError, "res_slot needs out_act='elu'",
     (B3, dict(out_act=RELU, out_pre_scaled=True, res=True, res_slot=SLOT)),
     (B3, dict(out_act=ELU, out_pre_scaled=True, res=True, res_slot=SLOT))),
    ("res_slot with two residuals", ValueError, "res_slot needs out_act='elu'",
     (B3, dict(out_act=ELU, out_pre_scaled=True, res=True, res2=True, res_slot=SLOT)),
     (B3, dict(out_act=ELU, out_pre_scaled=True, res=True, res_slot=SLOT))),
    ("out_pre_scaled with a residual (round 4)", ValueError, "out_pre_scaled cannot be combined with a residual",
     (B3, dict(out_act=ELU, out_pre_scaled=True, res=True)), (B3, dict(out_act=ELU, out_pre_scaled=True))),
    ("out_pre_scaled without out_act", ValueError, "out_pre_scaled without an output activation",
     (B3, dict(out_pre_scaled=True)), (B3, dict(out_act=ELU, out_pre_scaled=True))),
    ("out_act on the VALU kernel", ValueError, "fused output activations need the matrix-core path",
     (VALU, dict(out_act=ELU)), (NO_DGRAD, dict(out_act=ELU))),
    ("in_post on the VALU kernel", ValueError, "fused output activations need the matrix-core path",
     (VALU, dict(in_post=ELU)), (F32, dict(in_post=ELU))),
    ("gate off the bf16x3 kernel", ValueError, "gate= needs a bf16x3 convolution", (NO_DGRAD, dict(gate=ops.GATE_TANH)),
     (GATE, dict(gate=ops.GATE_TANH))),
    ("gate with two residuals", ValueError, "gate= needs a bf16x3 convolution",
     (GATE, dict(gate=ops.GATE_TANH, res=True, res2=True)), (GATE, dict(gate=ops.GATE_TANH, res=True))),
    ("gate with an output activation", ValueError, "gate= needs a bf16x3 convolution",
     (GATE, dict(gate=ops.GATE_IDENTITY, out_act=ELU)), (GATE, dict(gate=ops.GATE_IDENTITY))),
    ("gate_res of the full channel count", ValueError, "gate_res shape mismatch",
     (GATE, dict(gate=ops.GATE_TANH, gate_res=(N, 128, 16, 16))), (GATE, dict(gate=ops.GATE_TANH, gate_res=True))),
    ("in_sum without in_act='elu'", ValueError, "in_sum needs in_act='elu'", (DUAL, dict(in_sum=True, in_sum_slot=SLOT)),
     (DUAL, dict(in_act=ELU, in_sum=True, in_sum_slot=SLOT))),
    ("in_sum with skip aliases", ValueError, "in_sum needs in_act='elu'",
     (DUAL, dict(in_act=ELU, n_skip=1, in_sum=True, in_sum_slot=SLOT)), (DUAL, dict(in_act=ELU, in_sum=True, in_sum_slot=SLOT))),
    ("in_sum of another shape", ValueError, "in_sum needs in_act='elu'",
     (DUAL, dict(in_act=ELU, in_sum=(N, 64, 16, 8), in_sum_slot=SLOT)), (DUAL, dict(in_act=ELU, in_sum=True, in_sum_slot=SLOT))),
    ("in_sum on a 3x3 convolution", ValueError, "dual data gradient does not take",
     (B3, dict(in_act=ELU, in_sum=True, in_sum_slot=SLOT)), (DUAL, dict(in_act=ELU, in_sum=True, in_sum_slot=SLOT))),
    # the two that were raised in backward: everything they depend on is known at forward time
    ("in_act with in_post", ValueError, "in_act and in_post cannot both be set", (B3, dict(in_act=RELU, in_post=ELU)),
     (B3, dict(in_post=ELU))),
    ("in_act with in_post, no gradient wanted", ValueError, "in_act and in_post cannot both be set",
     (B3, dict(in_act=RELU, in_post=ELU, need_dx=False)), (B3, dict(in_act=RELU, need_dx=False))),
    ("in_post without a matrix-core data gradient", RuntimeError, "in_post needs the matrix-core data gradient",
     (NO_DGRAD, dict(in_post=ELU)), (NO_DGRAD, dict(in_post=ELU, need_dx=False))),
]


@pytest.mark.parametrize("line", REFUSALS, ids=lambda line: line[0])
def test_every_refusal_of_the_protocol_check_and_its_nearest_allowed_call(line):
    _, exc, fragment, (problem, refused), (ok_problem, allowed) = line
    with pytest.raises(exc) as e:
        _check(problem, **refused)
    assert type(e.value) is exc and fragment in str(e.value)
    _check(ok_problem, **allowed)


def test_the_record_asks_for_the_data_gradient_format_only_when_x_needs_a_gradient():
    assert _check(B3).fmt_t == ops.CONV_FMT_B3 and _check(B3, need_dx=False).fmt_t == 0
    call = _check(B3, need_dx=False, out_act=ELU, res=True)
    assert (call.fmt, call.has_res, call.has_res2, call.need_dx, call.gw) == (ops.CONV_FMT_B3, True, False, False, None)
    with pytest.raises(AttributeError):
        call.fmt = 0  # immutable: backward reads what forward checked


# ---- nn.Conv2d.forward up to the launch ------------------------------------------------------------------------------
@pytest.fixture
def launches(monkeypatch):
    """Lets Conv2d.forward run on CPU tensors as far as the kernels: tensors report is_cuda (the availability helpers ask),
    and the launching functions behind the glue are stand-ins that return tensors of the right shape and append what
    they were asked to the returned list — ("conv", call record) / ("act",) / ("add",) / ("down2",) / ("out_head",)."""
    log = []

    def conv_forward(ctx, call, x, weight, *operands):
        log.append(("conv", call))
        c = weight.shape[0] // 2 if call.gate is not None else weight.shape[0]
        y = x.new_empty((x.shape[0], c) + call.out_hw)
        return (y,) + tuple(x.view_as(x) for _ in range(call.n_skip)) if call.n_skip else y

    def stand_in(tag, shape_of):
        def fn(*args, **kwargs):
            log.append((tag,))
            return torch.empty_like(shape_of(*args))
        return fn

    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda t: True))
    monkeypatch.setattr(opconv, "_conv_forward", conv_forward)
    monkeypatch.setattr(ops, "add", stand_in("add", lambda a, b: a))
    monkeypatch.setattr(ops._Act, "apply", stand_in("act", lambda y, act: y))
    monkeypatch.setattr(pg_nn.Conv2d, "_forward_down2", stand_in("down2", lambda self, x, in_act, res: x[:, :, ::2, ::2]))
    monkeypatch.setattr(ops, "gpt_out_head_supported", lambda x, ln, conv: True)
    monkeypatch.setattr(ops, "gpt_out_head", stand_in("out_head", lambda x, ln, conv, chain: x))
    return log


@pytest.mark.parametrize("shape", PROTOCOL_SHAPES, ids=lambda s: s[0])
def test_protocol_matrix_refuses_exactly_what_the_gpu_matrix_refuses(launches, shape):
    """The loop of tests/test_gpu_ops.py::test_conv_protocol_matrix — in_act x (out_act, paired) x n_skip x res through
    conv2(A(conv1(act(x))) [+ r1]) + skips — as far as the launches: the same rule (a combination is refused if and only if
    it pairs the activation without matrix-core kernels on both convolutions, or with a residual behind it) and the same
    counts, with pair_ok taken from the format query. What ran asked the kernels for what was requested, fused or as
    separate launches."""
    name, n, c, h, w, cmid, k = shape
    conv1, conv2 = pg_nn.Conv2d(c, cmid, k, padding=1), pg_nn.Conv2d(cmid, c, 1)
    pair_ok = (all(ops.conv_formats(conv1.weight.shape, conv1._conv_spec(), (h, w), (h, w)))
               and all(ops.conv_formats(conv2.weight.shape, conv2._conv_spec(), (h, w))))
    x = torch.zeros(n, c, h, w, requires_grad=True)
    r1 = torch.zeros(n, cmid, h, w)
    bad, refused, ran = [], 0, 0
    for in_act, (out_act, paired), n_skip, use_r1 in itertools.product(
            (None, "relu", "elu"), ((None, False), ("elu", False), ("elu", True)), (0, 1, 2), (False, True)):
        combo = f"in_act={in_act} out_act={out_act} paired={paired} n_skip={n_skip} res={use_r1}"
        del launches[:]
        try:
            out = conv1(x, crop=(h, w), in_act=in_act, out_act=out_act, out_pre_scaled=paired, n_skip=n_skip,
                        res=r1 if use_r1 else None)
            y, aliases = (out[0], list(out[1:])) if n_skip else (out, [])
            kw = {"in_post": "elu"} if paired else {}
            z = conv2(y, **dict(zip(("res", "res2"), aliases)), **kw)
        except ValueError as e:
            if not (paired and (not pair_ok or use_r1)):
                bad.append(f"{combo}: unexpected ValueError: {e}")
            refused += 1
            continue
        ran += 1
        (_, call1), (_, call2) = [entry for entry in launches if entry[0] == "conv"]
        unfused = [entry[0] for entry in launches if entry[0] != "conv"]
        acts = unfused.count("act") + (call1.out_act != ops.ACT_NONE)
        adds = unfused.count("add") + call1.has_res + call2.has_res + call2.has_res2
        if (z.shape != x.shape or len(aliases) != n_skip or acts != (out_act is not None) or adds != use_r1 + n_skip
                or (call1.out_pre_scaled, call2.in_post != ops.ACT_NONE) != (paired, paired)
                or call1.in_act != pg_nn.convolution._ACTS[in_act] or call1.n_skip not in (0, n_skip)):
            bad.append(f"{combo}: conv1 {call1}, conv2 {call2}, separate launches {unfused}")
    assert not bad, f"{name}: {len(bad)} protocol combinations wrong:\n" + "\n".join(bad[:20])
    assert ran >= 36, f"{name}: only {ran} combinations ran ({refused} refused)"
    assert refused == (9 if pair_ok else 18), f"{name}: {refused} refusals, pair_ok={pair_ok}"


def _conv(problem, **kwargs):
    (cout, cin, kh, kw), spec, in_hw, _ = problem
    conv = pg_nn.Conv2d(cin, cout, (kh, kw), padding=(spec.pad_h, spec.pad_w), **kwargs)
    return conv, torch.zeros((N, cin) + in_hw, requires_grad=True)


def _like_out(problem, channels=None):
    return torch.zeros((N, channels or problem[0][0]) + problem[3])


def test_every_refusal_of_conv2d_forward_and_its_nearest_allowed_call(launches):
    """One line per `raise` of nn.Conv2d.forward: the call that triggers it, then the nearest call it lets through to the
    kernels."""
    ln = torch.nn.LayerNorm(64)
    conv, x = _conv(DUAL)
    with pytest.raises(ValueError, match="pre_ln= needs a plain 1x1 convolution"):
        conv(x, pre_ln=ln, in_act="elu")
    conv(x, pre_ln=ln)
    assert launches == [("out_head",)]

    r = torch.zeros_like(x)
    with pytest.raises(ValueError, match="res_slot / in_sum need the plain matrix-core training path"):
        conv(x, in_act="elu", in_sum=(r, SLOT), n_skip=1)
    del launches[:]
    conv(x, in_act="elu", in_sum=(r, SLOT))
    (_, call), = launches
    assert call.has_in_sum and call.in_sum_slot is SLOT and call.in_act == ELU

    conv, x = _conv(GATE)
    with pytest.raises(ValueError, match=r"gate= needs a convolution \(at most one residual\)"):
        conv(x, crop=GATE[3], gate=ops.GATE_TANH, out_act="elu")
    with pytest.raises(ValueError, match=r"gate= needs a convolution \(at most one residual\)"):
        narrow, xn = _conv(NO_DGRAD)
        narrow(xn, gate=ops.GATE_TANH)
    del launches[:]
    y, alias = conv(x, crop=GATE[3], gate=ops.GATE_TANH, res=_like_out(GATE), gate_res=_like_out(GATE, 64), n_skip=1)
    (_, call), = launches
    assert (call.gate, call.has_res, call.has_gate_res, call.n_skip, y.shape[1]) == (ops.GATE_TANH, True, True, 1, 64)

    down = pg_nn.Conv2d(8, 16, 4, stride=2, padding=1)
    xd = torch.zeros(N, 8, 16, 16, requires_grad=True)
    with pytest.raises(ValueError, match="fused output activations are not available for stride 2"):
        down(xd, out_act="elu")
    del launches[:]
    y, alias = down(xd, in_act="elu", res2=torch.zeros(N, 8, 8, 8), n_skip=1)
    assert launches == [("down2",), ("add",)] and alias is xd

    for problem, kw in ((NO_DGRAD, dict(in_post="elu")), (NO_DGRAD, dict(out_act="elu", out_pre_scaled=True)),
                        (VALU, dict(out_act="elu", out_pre_scaled=True))):
        conv, x = _conv(problem)
        with pytest.raises(ValueError, match="out_pre_scaled / in_post need the matrix-core path for this shape"):
            conv(x, **kw)
    conv, x = _conv(B3)
    del launches[:]
    conv(x, in_post="elu", out_act="elu", out_pre_scaled=True)
    (_, call), = launches
    assert (call.in_post, call.out_act, call.out_pre_scaled) == (ELU, ELU, True)


def test_conv2d_forward_runs_what_the_kernels_do_not_fuse_in_a_fixed_order(launches):
    """The unfused remainder behind the one conv2d_taps call: activation, res, res2, then the aliases — on a shape without
    matrix-core kernels everything is separate, on a bf16x3 shape with >= 64 output channels nothing is."""
    conv, x = _conv(VALU)
    res, res2 = _like_out(VALU), _like_out(VALU)
    y, a1, a2 = conv(x, out_act="elu", res=res, res2=res2, n_skip=2)
    (_, call), *rest = launches
    assert rest == [("act",), ("add",), ("add",)] and a1 is x and a2 is x
    assert not (call.has_res or call.has_res2 or call.n_skip or call.out_act)

    del launches[:]
    conv, x = _conv(B3)
    y, a1, a2 = conv(x, out_act="elu", res=_like_out(B3), res2=_like_out(B3), n_skip=2)
    (_, call), = launches
    assert (call.has_res, call.has_res2, call.n_skip, call.out_act) == (True, True, 2, ELU) and a1 is not x

    del launches[:]
    with torch.no_grad():
        x0 = x.detach()
        y, a1 = conv(x0, res=_like_out(B3), n_skip=1)  # no gradient wanted: a plain alias, no pass-through node
    (_, call), = launches
    assert call.n_skip == 0 and not call.need_dx and call.fmt_t == 0 and a1 is x0


# ---- the memoised format helper ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
def test_conv_formats_equals_the_library_query_and_asks_it_once(lib, monkeypatch, seed):
    """conv_formats over a seeded sweep of problems (kernel, padding, causal / random tap lists, channel counts, extents,
    crops) equals pg_conv_mfma_supported asked directly for both orientations; asking again reaches the library no more."""
    asked = []
    query = lib.pg_conv_mfma_supported

    def counted(*args):
        asked.append(args)
        return query(*args)

    r = random.Random(seed)
    kernels = [(1, 1), (2, 2), (3, 3), (2, 3), (1, 3), (3, 1), (2, 1), (1, 2), (5, 5), (4, 4), (7, 7), (3, 5)]
    problems = []
    while len(problems) < 300:
        kh, kw = r.choice(kernels)
        ph, pw = r.choice([(0, 0), (kh // 2, kw // 2), (kh - 1, kw - 1), (kh - 1, kw // 2)])
        taps = [(u, v) for u in range(kh) for v in range(kw)]
        mode = r.choice(["all", "A", "B", "random"])
        if mode == "A":
            taps = [(u, v) for u, v in taps if u < kh // 2 or (u == kh // 2 and v < kw // 2)] or taps
        elif mode == "B":
            taps = [(u, v) for u, v in taps if u < kh // 2 or (u == kh // 2 and v <= kw // 2)]
        elif mode == "random":
            taps = [t for t in taps if r.random() < 0.6] or taps
        cin = r.choice([1, 2, 3, 4, 5, 7, 8, 12, 16, 24, 32, 33, 40, 48, 64, 66, 69, 96, 100, 128, 160, 192, 256, 320, 512])
        cout = r.choice([1, 2, 3, 8, 10, 16, 24, 32, 36, 40, 56, 64, 72, 96, 100, 128, 160, 192, 256, 320, 512])
        ih = r.choice([1, 2, 3, 4, 5, 7, 8, 12, 14, 16, 20, 28, 32, 33, 48, 64, 100, 128])
        iw = r.choice([1, 2, 3, 4, 6, 8, 12, 14, 16, 20, 28, 32, 36, 48, 64, 100, 128, 256, 300])
        spec = ops.ConvSpec(kh, kw, ph, pw, active=taps)
        oh, ow = spec.full_out(ih, iw)
        if r.random() < 0.3:
            oh, ow = min(oh, ih), min(ow, iw)  # a crop
        if oh >= 1 and ow >= 1:
            problems.append(((cout, cin, kh, kw), spec, (ih, iw), (oh, ow)))
    formats = set()
    for wshape, spec, (ih, iw), (oh, ow) in problems:
        t, (cout, cin) = len(spec.fwd_taps), wshape[:2]
        want = (query(cin, cout, t, oh, ow, iw, spec.hr, spec.hc), query(cout, cin, t, ih, iw, ow, spec.hr, spec.hc))
        assert ops.conv_formats(wshape, spec, (ih, iw), (oh, ow)) == want, (wshape, spec.fwd_taps, ih, iw, oh, ow)
        formats.add(want)
    assert {f for pair in formats for f in pair} == {0, ops.CONV_FMT_F32, ops.CONV_FMT_B3}, formats
    monkeypatch.setattr(lib, "pg_conv_mfma_supported", counted)
    for wshape, spec, in_hw, out_hw in problems:  # answered above: the library is not asked
        ops.conv_formats(wshape, spec, in_hw, out_hw)
        opconv._resolve(wshape, spec, in_hw, out_hw, True)
        ops._use_mfma(lib, wshape[1], wshape[0], spec, out_hw, in_hw[1])
    assert not asked
    fresh = ops.ConvSpec(3, 3, 1, 1)  # the answers belong to the tap list: another ConvSpec asks for itself, once each way
    first = ops.conv_formats((64, 128, 3, 3), fresh, (16, 16))
    assert len(asked) == 2 and ops.conv_formats((64, 128, 3, 3), fresh, (16, 16)) == first and len(asked) == 2
    assert ops.conv_formats((64, 128, 3, 3), fresh, (16, 16), dgrad=False) == (first[0], 0) and len(asked) == 2
