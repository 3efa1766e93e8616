"""GPU: the code-index convolution kernels (csrc/code_conv.hip) against the float64 reference of tests/_code_conv_ref.py.

Gates are the project's own: _util.assert_close at 1e-4 for outputs, _util.GradReport (1e-4 / 5e-6) for gradients; the
measured worst errors are printed and sit orders below (fp32 sums of at most a few thousand terms). The bit-level
properties (run-to-run, accumulate, exact halving, band = row of the full call, lookup) are asserted with torch.equal."""

import pytest
import torch

import _code_conv_ref as ref
import _util

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
OUT_TOL = 1e-4

SHAPES = [
    # (N, K, Cout, H, W, kernel, mask)
    (2, 5, 6, 3, 5, 7, "A"),       # every tap crosses a border, Cout no multiple of 4
    (3, 512, 64, 8, 8, 3, "A"),
    (2, 4096, 16, 4, 4, 3, "B"),
    (2, 7, 1, 1, 9, 3, "A"),
]


def _sid(s):
    return "n{}_k{}_c{}_{}x{}_k{}{}".format(*s)


def _spec(ks, mask):
    from pytorch_generative_amd import ops

    m = ref.causal_mask(ks, ks, mask == "A")
    taps = [(u, v) for u in range(ks) for v in range(ks) if m[u, v] != 0]
    return ops.ConvSpec(ks, ks, ks // 2, ks // 2, active=taps, wgrad_all=True), m


def _inputs(shape, seed=0, codes=None):
    n, k, cout, h, w, ks, mask = shape
    g = torch.Generator().manual_seed(seed)
    if codes is None:
        codes = torch.randint(0, k, (n, 1, h, w), generator=g)
    spec, m = _spec(ks, mask)
    weight = torch.randn(cout, k, ks, ks, generator=g) * m.float()  # the caller has masked it
    bias = torch.randn(cout, generator=g)
    dy = torch.randn(n, cout, h, w, generator=g)
    return codes, weight, bias, dy, spec


def _gpu(codes, weight, bias, dy, spec, k):
    from pytorch_generative_amd import ops

    w = weight.to(DEV).requires_grad_(True)
    b = bias.to(DEV).requires_grad_(True)
    out = ops.code_conv2d(ref.to_levels(codes, k).to(DEV), w, b, spec, k)
    out.backward(dy.to(DEV))
    torch.cuda.synchronize()
    return out.detach(), w.grad, b.grad


def _want(codes, weight, bias, dy, shape):
    n, k, cout, h, w, ks, _ = shape
    pad = (ks // 2, ks // 2)
    if n * h * w * ks * ks <= 5000:  # the loops themselves
        return (ref.forward(codes, weight, bias, pad),) + ref.wgrad(codes, dy, k, (ks, ks), pad)
    return (ref.dense(codes, weight, bias, pad),) + ref.dense_wgrad(codes, dy, k, (ks, ks), pad)


def _compare(what, got, want):
    out, dw, db = got
    e = _util.rel_err(out, want[0])
    print(f"[code_conv] {what}: output rel err {e:.3e}")
    assert e <= OUT_TOL, f"{what}: output rel err {e:.3e}"
    rep = _util.GradReport(what)
    rep.add("weight", dw, want[1])
    rep.add("bias", db, want[2])
    rep.finish()


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_forward_and_gradients_match_float64(shape):
    codes, weight, bias, dy, spec = _inputs(shape)
    got = _gpu(codes, weight, bias, dy, spec, shape[1])
    _compare(_sid(shape), got, _want(codes, weight, bias, dy, shape))
    used = torch.zeros(shape[1], dtype=torch.bool)
    used[codes.flatten()] = True
    if not used.all():  # codes that never occur: exact zeros
        assert not got[1][:, (~used).to(DEV)].any()


@pytest.mark.parametrize("kind", ["unknown", "one_code", "few_codes"])
def test_special_code_images(kind):
    shape = (3, 512, 64, 8, 8, 3, "A")
    n, k, cout, h, w, ks, _ = shape
    g = torch.Generator().manual_seed(3)
    if kind == "unknown":
        codes = torch.randint(0, k, (n, 1, h, w), generator=g)
        codes[torch.rand(codes.shape, generator=g) < 0.4] = -1
    elif kind == "one_code":  # the longest list
        codes = torch.full((n, 1, h, w), 77)
    else:
        codes = torch.randint(0, 3, (n, 1, h, w), generator=g) * 200  # 0, 200, 400
    codes, weight, bias, dy, spec = _inputs(shape, codes=codes)
    got = _gpu(codes, weight, bias, dy, spec, k)
    _compare(kind, got, _want(codes, weight, bias, dy, shape))
    used = torch.zeros(k, dtype=torch.bool)
    used[codes[codes >= 0]] = True
    assert int((~used).sum()) > k // 2
    assert not got[1][:, (~used).to(DEV)].any(), "rows of unused codes are not exact zeros"


@pytest.mark.parametrize("kind", ["random", "one_code"])
def test_long_lists_are_merged_in_chunks(kind):
    from pytorch_generative_amd import ops

    shape = (64, 32, 8, 16, 16, 3, "A")
    n, k, cout, h, w, ks, _ = shape
    max_chunks, items = ops.code_conv_wgrad_plan(n, k, h, w)
    assert max_chunks >= 2 and items >= k + 2
    codes = torch.full((n, 1, h, w), 5) if kind == "one_code" else None
    codes, weight, bias, dy, spec = _inputs(shape, seed=4, codes=codes)
    counts = torch.bincount(codes.flatten(), minlength=k)
    assert int(counts.max()) > 512, "no list longer than one chunk"
    got = _gpu(codes, weight, bias, dy, spec, k)
    _compare(f"merge {kind}", got, _want(codes, weight, bias, dy, shape))


def _wgrad_raw(levels, dy, dw, db, accumulate, shape):
    from pytorch_generative_amd import _lib, ops

    lib = _lib.load()
    n, k, cout, h, w, ks, _ = shape
    ws_n = lib.pg_code_conv_wgrad_workspace_floats(n, k, h, w, cout, ks, ks)
    ws = torch.empty(ws_n, device=DEV)
    _lib.check(lib.pg_code_conv_wgrad(levels.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr(), accumulate, n, k, h, w,
                                      cout, ks, ks, h, w, ks // 2, ks // 2, ws.data_ptr(), ws_n, ops._stream()),
               "pg_code_conv_wgrad")


@pytest.mark.parametrize("shape", [(64, 32, 8, 16, 16, 3, "A"), (3, 512, 64, 8, 8, 3, "A"), (2, 5, 6, 3, 5, 7, "A")], ids=_sid)
def test_backward_bit_level_properties(shape):
    n, k, cout, h, w, ks, _ = shape
    codes, _, _, dy, _ = _inputs(shape, seed=6)
    levels, dy = ref.to_levels(codes, k).to(DEV), dy.to(DEV)

    def run(dy, accumulate=0, fill=None):
        dw = torch.full((cout, k, ks, ks), float("nan"), device=DEV) if fill is None else fill[0].clone()
        db = torch.full((cout,), float("nan"), device=DEV) if fill is None else fill[1].clone()
        _wgrad_raw(levels, dy, dw, db, accumulate, shape)
        return dw, db

    dw, db = run(dy)
    dw2, db2 = run(dy)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "two runs differ"
    g = torch.Generator().manual_seed(7)
    fill = (torch.randn(dw.shape, generator=g).to(DEV), torch.randn(db.shape, generator=g).to(DEV))
    dwa, dba = run(dy, accumulate=1, fill=fill)
    assert torch.equal(dwa, fill[0] + dw) and torch.equal(dba, fill[1] + db), "accumulate is not one fp32 add"
    dwh, dbh = run(dy * 0.5)
    assert torch.equal(dwh, dw * 0.5) and torch.equal(dbh, db * 0.5), "half the gradient is not exactly half"


def test_band_and_window_equal_rows_of_the_full_call():
    from pytorch_generative_amd import ops

    shape = (3, 16, 12, 6, 7, 7, "A")
    n, k, cout, h, w, ks, _ = shape
    codes, weight, bias, _, spec = _inputs(shape, seed=8)
    wd, bd = weight.to(DEV), bias.to(DEV)
    levels = ref.to_levels(codes, k).to(DEV)
    with torch.no_grad():
        full = ops.code_conv2d(levels, wd, bd, spec, k)
        first = ops.code_conv2d(levels, wd, bd, spec, k, out_hw=(1, w))
        assert torch.equal(first[:, :, 0], full[:, :, 0])
        reach = ks // 2
        band_spec = ops.ConvSpec(ks, ks, spec.pad_h - reach, spec.pad_w, active=spec.fwd_taps)
        for row in range(h):
            band = torch.full((n, 1, reach + 1, w), -1.0, device=DEV)
            lo = max(0, row - reach)
            band[:, :, reach + 1 - (row + 1 - lo):] = levels[:, :, lo:row + 1]
            got = ops.code_conv2d(band, wd, bd, band_spec, k, out_hw=(1, w))
            assert torch.equal(got[:, :, 0], full[:, :, row]), f"row {row}"


@pytest.mark.parametrize("n,k,d,h,w", [(2, 4, 4, 2, 2), (3, 512, 64, 8, 8), (1, 4096, 5, 3, 7)])
def test_vq_lookup_is_a_copy(n, k, d, h, w):
    from pytorch_generative_amd import ops

    g = torch.Generator().manual_seed(9)
    emb = torch.randn(k, d, generator=g).to(DEV)
    idx = torch.randint(0, k, (n, 1, h, w), generator=g)
    idx[0, 0, 0, 0], idx[-1, 0, -1, -1] = k - 1, 0
    got = ops.vq_lookup(ops.codes_to_levels(idx, k).to(DEV), emb)
    want = emb[idx[:, 0].to(DEV)].permute(0, 3, 1, 2)
    assert got.shape == (n, d, h, w) and torch.equal(got, want)


@pytest.mark.parametrize("use_dev", [False, True])
def test_sample_embed_codes_equals_the_stem_column(use_dev):
    from pytorch_generative_amd import _lib, ops

    lib = _lib.load()
    shape = (5, 16, 12, 4, 6, 3, "A")
    n, k, cout, h, w, ks, _ = shape
    codes, weight, bias, _, spec = _inputs(shape, seed=10)
    codes[torch.rand(codes.shape, generator=torch.Generator().manual_seed(11)) < 0.2] = -1
    pos_term = torch.randn(cout, h, w, generator=torch.Generator().manual_seed(12)).to(DEV)
    wd, bd = weight.to(DEV), bias.to(DEV)
    levels = ref.to_levels(codes, k).to(DEV)
    with torch.no_grad():
        full = ops.code_conv2d(levels, wd, bd, spec, k) + pos_term
    want64 = ref.forward(codes, weight, bias, (1, 1)) + pos_term.double().cpu()
    ld = 16
    for r, c in [(0, 0), (1, w - 1), (h - 1, w - 1)]:
        out = torch.zeros(cout, ld, device=DEV)
        pos_dev = torch.tensor([r * w + c], dtype=torch.int32, device=DEV)
        _lib.check(lib.pg_sample_embed_codes(levels.data_ptr(), wd.data_ptr(), bd.data_ptr(), pos_term.data_ptr(),
                                             out.data_ptr(), n, k, h, w, cout, ks, ks, 0 if use_dev else r,
                                             0 if use_dev else c, ld, pos_dev.data_ptr() if use_dev else 0, ops._stream()),
                   "pg_sample_embed_codes")
        torch.cuda.synchronize()
        got = out[:, :n].t()
        e = max(_util.rel_err(got, full[:, :, r, c]), _util.rel_err(got, want64[:, :, r, c]))
        print(f"[code_conv] sample_embed_codes ({r}, {c}) dev={use_dev}: rel err {e:.3e}")
        assert e <= OUT_TOL
        assert not out[:, n:].any()
