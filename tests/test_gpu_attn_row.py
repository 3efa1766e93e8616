"""GPU: the row-query attention kernel of the row-cached sampler (csrc/attention_row.hip: pg_attn_row, pg_row_gather) through
the C-ABI, against the float64 restatement of tests/_attn_row_ref.py (itself pinned to the oracle on the CPU by
tests/test_attn_row_cpu.py).

The bound is the project's for the sampler kernels: _util.assert_close at 1e-5; everything stated as unchanged, equal between
two paths, or zero is bit-equality. Cache rows >= r are NaN in every comparison with the reference: a finite result within
the bound is the proof that the launch reads none of them."""

import pytest
import torch

import _attn_row_ref as aref
import _util

pytestmark = pytest.mark.gpu

GUARD = 256            # sentinel floats on either side of every buffer the kernel writes
GUARD_VALUE = 54321.0
NAN = float("nan")


def _sid(shape):
    return "-".join(map(str, shape))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from pytorch_generative_amd import _lib

    _lib.load()  # fail loudly if the extension is missing
    return torch.device("cuda:0")


class _Guarded:
    """A device copy of `t` with GUARD sentinel floats before and after it in one allocation."""

    def __init__(self, t, dev):
        self.flat = torch.full((t.numel() + 2 * GUARD,), GUARD_VALUE, device=dev)
        self.t = self.flat[GUARD:GUARD + t.numel()].view(t.shape)
        self.t.copy_(t)

    def intact(self):
        want = torch.full((GUARD,), GUARD_VALUE)
        return torch.equal(self.flat[:GUARD].cpu(), want) and torch.equal(self.flat[-GUARD:].cpu(), want)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _launch(q_row, kv_row, kc, vc, out, heads, r, mask_center, write_cache, row_dev=None):
    """The raw status of pg_attn_row on device tensors, called as ops.attention_row calls it."""
    from pytorch_generative_amd import _lib

    n, e, h, w = kc.shape
    o = vc.shape[1]
    assert q_row.shape == (n, e, 1, w) and kv_row.shape == (n, e + o, 1, w) and vc.shape == (n, o, h, w)
    assert out.shape == (n, o, 1, w) and all(t.is_contiguous() for t in (q_row, kv_row, kc, vc, out))
    return _lib.load().pg_attn_row(q_row.data_ptr(), kv_row.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), n, heads,
                                   e // heads, o // heads, h, w, r, mask_center, write_cache,
                                   None if row_dev is None else row_dev.data_ptr(), torch.cuda.current_stream().cuda_stream)


def _run(dev, q_row, kv_row, kc, vc, heads, r, mask_center, write_cache=1, row_dev=None):
    """One guarded launch from host tensors; (out, k_cache, v_cache) on the host after checking every sentinel."""
    from pytorch_generative_amd import _lib

    n, o, w = kc.shape[0], vc.shape[1], kc.shape[3]
    out, kcd, vcd = _Guarded(torch.full((n, o, 1, w), NAN), dev), _Guarded(kc, dev), _Guarded(vc, dev)
    _lib.check(_launch(q_row.to(dev), kv_row.to(dev), kcd.t, vcd.t, out.t, heads, r, mask_center, write_cache, row_dev),
               "pg_attn_row")
    torch.cuda.synchronize()
    assert out.intact() and kcd.intact() and vcd.intact(), "written outside a buffer"
    return out.t.cpu(), kcd.t.cpu(), vcd.t.cpu()


def _check_image(dev, shape, q, kv, mask_center, what):
    """Every row of the image (q, kv): the launch on NaN-poisoned caches against the float64 helper, and its cache write."""
    n, heads, dk, dv, h, w = shape
    e = heads * dk
    for r in range(h):
        q_row, kv_row, kc, vc = aref.row_inputs(q, kv, e, r, fill=NAN)
        want = aref.attn_row_ref(q_row, kv_row, torch.nan_to_num(kc), torch.nan_to_num(vc), heads, r, mask_center)[0]
        got, kc2, vc2 = _run(dev, q_row, kv_row, kc, vc, heads, r, mask_center)
        assert bool(torch.isfinite(got).all()), f"{what} r={r}: a cache row >= r was read"
        err = _util.rel_err(got, want) if float(want.abs().max()) > 0 else float(got.abs().max())
        print(f"[attn_row] {what} mask_center={mask_center} r={r}: rel err {err:.3e}")
        if float(want.abs().max()) > 0:
            _util.assert_close(got, want, aref.TOL, f"{what} r={r}")
        if mask_center and r == 0:  # no key admitted: exactly 0
            assert float(got[:, :, 0, 0].abs().max()) == 0.0
            if w == 1:
                assert float(got.abs().max()) == 0.0
        # cache row r is kv_row bit for bit; every other row keeps its bits (NaN included)
        assert torch.equal(kc2[:, :, r], kv_row[:, :e, 0]) and torch.equal(vc2[:, :, r], kv_row[:, e:, 0])
        kc2[:, :, r], vc2[:, :, r] = kc[:, :, r], vc[:, :, r]
        assert _same_bits(kc2, kc) and _same_bits(vc2, vc), f"{what} r={r}: a cache row other than r was written"


@pytest.mark.parametrize("mask_center", [0, 1])
@pytest.mark.parametrize("shape", aref.SHAPES, ids=_sid)
def test_rows_against_float64(dev, shape, mask_center):
    q, kv = aref.case(shape)
    _check_image(dev, shape, q, kv, mask_center, f"shape {shape}")


@pytest.mark.parametrize("mask_center", [0, 1])
def test_one_row_past_the_key_tile(dev, lib, mask_center):
    """H * W exceeds the plan's key tile by one row: the last row's cached keys fill one tile exactly and the row's own keys
    open another; the row before it ends inside the first tile."""
    from pytorch_generative_amd import ops

    heads, dk, dv, w = 1, 4, 8, 8
    tile = ops.attention_row_plan(heads, dk, dv, 2, w)["key_tile"]
    assert tile % w == 0, "pick a row length that divides the key tile"
    h = tile // w + 1
    assert ops.attention_row_plan(heads, dk, dv, h, w)["key_tile"] == tile and h * w == tile + w
    shape = (2, heads, dk, dv, h, w)
    q, kv = aref.case(shape, seed=3)
    _check_image(dev, shape, q, kv, mask_center, f"tile {tile} shape {shape}")


@pytest.mark.parametrize("where", [(0, 0), (2, 3)], ids=["first", "last-row"])
@pytest.mark.parametrize("mask_center", [0, 1])
def test_scores_of_size_80(dev, mask_center, where):
    """Scores ~80 on one key: the maximum is subtracted, and a running maximum that jumps by ~100 rescales what came before."""
    shape = (2, 1, 4, 32, 3, 5)
    q, kv = aref.spike_case(shape, where)
    _check_image(dev, shape, q, kv, mask_center, f"spike at {where}")


def test_spike_in_a_later_tile(dev):
    """The spiked key lies behind the first key tile: the accumulators of the first tile are rescaled to nothing."""
    from pytorch_generative_amd import ops

    heads, dk, dv, w = 1, 4, 8, 8
    tile = ops.attention_row_plan(heads, dk, dv, 2, w)["key_tile"]
    h = tile // w + 2
    shape = (1, heads, dk, dv, h, w)
    q, kv = aref.spike_case(shape, (h - 2, 1), seed=1)
    e = heads * dk
    r = h - 1
    q_row, kv_row, kc, vc = aref.row_inputs(q, kv, e, r, fill=NAN)
    want = aref.attn_row_ref(q_row, kv_row, torch.nan_to_num(kc), torch.nan_to_num(vc), heads, r, 1)[0]
    got = _run(dev, q_row, kv_row, kc, vc, heads, r, 1)[0]
    assert bool(torch.isfinite(got).all())
    _util.assert_close(got, want, aref.TOL, "spike in the second tile")


@pytest.mark.parametrize("shape", [aref.SHAPES[0], aref.SHAPES[1]], ids=_sid)
def test_write_cache_off_leaves_the_caches(dev, shape):
    n, heads, dk, dv, h, w = shape
    e = heads * dk
    q, kv = aref.case(shape, seed=5)
    for r in range(h):
        q_row, kv_row, kc, vc = aref.row_inputs(q, kv, e, r, fill=NAN)
        on = _run(dev, q_row, kv_row, kc, vc, heads, r, 1, write_cache=1)[0]
        off, kc2, vc2 = _run(dev, q_row, kv_row, kc, vc, heads, r, 1, write_cache=0)
        assert _same_bits(kc2, kc) and _same_bits(vc2, vc)
        assert _same_bits(on, off)


@pytest.mark.parametrize("shape", [aref.SHAPES[1], aref.SHAPES[4]], ids=_sid)
def test_device_row_in_one_graph(dev, shape):
    """One hipGraph holding the single launch, replayed for r = 0 .. H-1 with only row_dev changed (and the row's inputs
    copied into the captured buffers): bit-equal to the eager launches with a host r, outputs and caches."""
    from pytorch_generative_amd import _lib

    n, heads, dk, dv, h, w = shape
    e, o = heads * dk, heads * dv
    q, kv = aref.case(shape, seed=7)
    qd, kvd = q.to(dev), kv.to(dev)

    def fresh():
        return (torch.zeros(n, e, h, w, device=dev), torch.zeros(n, o, h, w, device=dev),
                torch.empty(n, o, 1, w, device=dev))

    kc_e, vc_e, out_e = fresh()
    eager = []
    for r in range(h):
        _lib.check(_launch(qd[:, :, r:r + 1].contiguous(), kvd[:, :, r:r + 1].contiguous(), kc_e, vc_e, out_e, heads, r, 1, 1),
                   "pg_attn_row")
        eager.append(out_e.clone())
    kc_g, vc_g, out_g = fresh()
    q_in, kv_in = torch.zeros(n, e, 1, w, device=dev), torch.zeros(n, e + o, 1, w, device=dev)
    row_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture; write_cache off: the caches stay as they are
        _lib.check(_launch(q_in, kv_in, kc_g, vc_g, out_g, heads, 0, 1, 0, row_dev), "pg_attn_row")
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        # the host r is ignored when row_dev is given: h - 1 here, every row in the replays
        _lib.check(_launch(q_in, kv_in, kc_g, vc_g, out_g, heads, h - 1, 1, 1, row_dev), "pg_attn_row")
    for r in range(h):
        q_in.copy_(qd[:, :, r:r + 1])
        kv_in.copy_(kvd[:, :, r:r + 1])
        row_dev.fill_(r)
        graph.replay()
        assert _same_bits(out_g, eager[r]), f"row {r}"
    torch.cuda.synchronize()
    assert _same_bits(kc_g, kc_e) and _same_bits(vc_g, vc_e)
    assert torch.equal(kc_g.cpu(), kv[:, :e]) and torch.equal(vc_g.cpu(), kv[:, e:])
    # a stale device row is clamped into the image
    row_dev.fill_(h + 5)
    graph.replay()
    assert _same_bits(out_g, eager[h - 1])
    row_dev.fill_(-3)
    graph.replay()  # row 0 with the last row's inputs: rewrites cache row 0, restored below
    torch.cuda.synchronize()
    kc_g[:, :, 0].copy_(kc_e[:, :, 0])
    vc_g[:, :, 0].copy_(vc_e[:, :, 0])
    # nothing but row_dev changes between the replays: the same inputs and (full) caches for every row, nothing written
    graph0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph0):
        _lib.check(_launch(q_in, kv_in, kc_g, vc_g, out_g, heads, 0, 0, 0, row_dev), "pg_attn_row")
    for r in range(h):
        row_dev.fill_(r)
        graph0.replay()
        _lib.check(_launch(q_in, kv_in, kc_e, vc_e, out_e, heads, r, 0, 0), "pg_attn_row")
        assert _same_bits(out_g, out_e), f"row {r}, only row_dev changed"
    assert _same_bits(kc_g, kc_e) and _same_bits(vc_g, vc_e)


def test_reproducible_and_independent_of_the_batch(dev):
    """Two runs give the same bits, and sample 0 alone (N = 1) the bits it has inside a batch of 5."""
    shape = aref.SHAPES[1]
    n, heads, dk, dv, h, w = shape
    e = heads * dk
    q, kv = aref.case(shape, seed=9)
    for mask_center in (0, 1):
        for r in range(h):
            q_row, kv_row, kc, vc = aref.row_inputs(q, kv, e, r)
            a = _run(dev, q_row, kv_row, kc, vc, heads, r, mask_center)[0]
            b = _run(dev, q_row, kv_row, kc, vc, heads, r, mask_center)[0]
            one = _run(dev, q_row[:1], kv_row[:1], kc[:1], vc[:1], heads, r, mask_center)[0]
            assert _same_bits(a, b) and _same_bits(a[:1], one)


@pytest.mark.parametrize("shape", [(2, 3, 4, 5), (1, 2, 1, 1), (3, 2, 5, 65)], ids=_sid)
def test_row_gather_is_the_slice(dev, shape):
    from pytorch_generative_amd import _lib, ops

    n, c, h, w = shape
    g = torch.Generator().manual_seed(4)
    src = torch.randn(shape, generator=g).to(dev)
    row_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    for r in range(h):
        want = src[:, :, r:r + 1].contiguous()
        assert torch.equal(ops.row_gather(src, r), want)
        row_dev.fill_(r)
        assert torch.equal(ops.row_gather(src, row_dev), want)
        dst = _Guarded(torch.full((n, c, 1, w), NAN), dev)
        _lib.check(_lib.load().pg_row_gather(src.data_ptr(), dst.t.data_ptr(), n, c, h, w, r, None,
                                             torch.cuda.current_stream().cuda_stream), "pg_row_gather")
        torch.cuda.synchronize()
        assert dst.intact() and torch.equal(dst.t, want)


def test_operator_layer(dev):
    """ops.attention_row is the C-ABI call (same bits, host and device row) and refuses what it cannot run."""
    from pytorch_generative_amd import ops

    shape = aref.SHAPES[0]
    n, heads, dk, dv, h, w = shape
    e = heads * dk
    q, kv = aref.case(shape, seed=2)
    r = h - 1
    q_row, kv_row, kc, vc = aref.row_inputs(q, kv, e, r)
    want = _run(dev, q_row, kv_row, kc, vc, heads, r, 1)[0]
    kcd, vcd = kc.to(dev), vc.to(dev)
    got = ops.attention_row(q_row.to(dev), kv_row.to(dev), kcd, vcd, heads, True, row=r)
    assert _same_bits(got, want)
    assert torch.equal(kcd[:, :, r].cpu(), kv_row[:, :e, 0]) and torch.equal(vcd[:, :, r].cpu(), kv_row[:, e:, 0])
    row_dev = torch.full((1,), r, dtype=torch.int32, device=dev)
    got = ops.attention_row(q_row.to(dev), kv_row.to(dev), kcd, vcd, heads, True, row=row_dev, write_cache=False)
    assert _same_bits(got, want)
    with pytest.raises(RuntimeError):  # no CPU fallback
        ops.attention_row(q_row, kv_row, kc, vc, heads, True, row=r)
    with pytest.raises(ValueError):
        ops.attention_row(q_row.to(dev), kv_row.to(dev)[:, :-1], kcd, vcd, heads, True, row=r)
    with pytest.raises(ValueError):
        ops.attention_row(q_row.to(dev), kv_row.to(dev), kcd, vcd, heads, True, row=h)
    with pytest.raises(ValueError):
        ops.attention_row(q_row.to(dev), kv_row.to(dev), kcd, vcd, heads, True, row=torch.zeros(1, device=dev))
    with pytest.raises(ValueError):  # outside the planner's domain: an error, not another route
        ops.attention_row(torch.zeros(1, 65, 1, 2, device=dev), torch.zeros(1, 66, 1, 2, device=dev),
                          torch.zeros(1, 65, 2, 2, device=dev), torch.zeros(1, 1, 2, 2, device=dev), 1, True, row=0)
