"""GPU: the VectorQuantizer beyond its first half — the codebook trained by gradient descent (`use_ema=False`) and codes
wider than 64 (csrc/vq_mfma.hip: the tiled fp32-MFMA assignment, the fixed-order one-hot GEMM of the codebook gradient).
Against outputs of the reference (tests/golden/vq_quantizer.pt case `sgd_train`, tests/golden/vq_wide/ from
make_vq_wide_golden.py: every input there keeps a float64 tie margin, so indices are compared exactly), against float64 at
a shape where no margin can be arranged, bit reproducibility, the flat-gradient sink, graph replay, the wide VQ-VAE."""

import copy

import pytest
import torch

import _util
import _vq_wide

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _quantizer(k, d, use_ema, embedding=None, extra=None):
    import pytorch_generative_amd as pg

    m = pg.nn.VectorQuantizer(n_embeddings=k, embedding_dim=d, use_ema=use_ema)
    if embedding is not None:
        state = {"_embedding": embedding}
        state.update(extra or {})
        m.load_state_dict(state, strict=True)
    return m.to(DEV)


def test_gradient_codebook_matches_reference_golden():
    """Case `sgd_train` of vq_quantizer.pt (D = 8: the one-position-per-thread assignment + the new gradient)."""
    g = _util.load_golden("vq_quantizer")["cases"]["sgd_train"]
    assert list(g["before"]) == ["_embedding"] and not g["use_ema"]
    m = _quantizer(12, 8, False)
    m.load_state_dict(g["before"], strict=True)
    m.train(g["training"])
    x = g["x"].to(DEV).requires_grad_(True)
    q, loss = m(x)
    (q.sum() * 0.5 + loss).backward()
    assert torch.equal(q.detach().cpu(), g["quantized"]), "a different codebook row was chosen"
    _util.assert_close(loss, g["loss"], 1e-5, "commitment + embedding loss")
    rep = _util.GradReport("vq_quantizer sgd_train", tol=1e-5)
    rep.add("dx", x.grad, g["dx"])
    rep.add("d_embedding", m._embedding.grad, g["d_embedding"])
    rep.finish()
    assert isinstance(m._embedding, torch.nn.Parameter)
    assert torch.equal(m._embedding.detach().cpu(), g["before"]["_embedding"]), "forward must not move the parameter"
    # eval: the same loss (nn/utils.py:91-93 adds the embedding loss in both modes)
    m.eval()
    with torch.no_grad():
        q2, loss2 = m(g["x"].to(DEV))
    assert torch.equal(q2.cpu(), g["quantized"]) and torch.equal(loss2, loss.detach())


@pytest.mark.parametrize("use_ema", [False, True], ids=["sgd", "ema"])
@pytest.mark.parametrize("name", _vq_wide.case_names())
def test_wide_cases_match_reference(name, use_ema):
    c = _vq_wide.load_case(name)
    k, d = c["n_embeddings"], c["embedding_dim"]
    m = _quantizer(k, d, use_ema, c["embedding"], c["ema"]["before"] if use_ema else None)
    m.train()
    x = c["x"].to(DEV).requires_grad_(True)
    q, loss = m(x)
    (q.sum() * 0.5 + loss).backward()
    assert torch.equal(m.last_indices.cpu(), c["indices"]), f"{name}: indices differ from the reference's"
    assert torch.equal(q.detach().cpu(), c["quantized"]), f"{name}: quantized output is not bit-equal"
    if c["duplicate_rows"]:
        low, high = c["duplicate_rows"]
        got = m.last_indices.cpu()
        assert bool((got == low).any()) and not bool((got == high).any()), "the lower of two identical rows must win"
    _util.assert_close(loss, c["loss_ema" if use_ema else "loss_sgd"], 1e-5, f"{name} loss")
    rep = _util.GradReport(f"vq_wide {name} {'ema' if use_ema else 'sgd'}")
    rep.add("dx", x.grad, c["dx"])
    if use_ema:
        rep.finish()
        for key, want in c["ema"]["after"].items():
            _util.assert_close(m.state_dict()[key], want, 1e-5, f"{name} buffer {key} after forward")
    else:
        rep.add("d_embedding", m._embedding.grad, c["d_embedding"])
        rep.finish()
        assert torch.equal(m._embedding.detach().cpu(), c["embedding"])


def test_op_parity_float64_without_margin():
    """P = 1100, D = 130, K = 300 (_vq_wide.ragged_problem): near-ties exist, so an index is accepted if and only if its
    float64 distance is within the tie margin of the best, and at most 1 % of the positions may differ from the float64
    argmin at all (test_vq_codebook_cpu.py checks that torch's own fp32 evaluation stays inside that cap on this seed).
    The gradients are compared with float64 values recomputed from the indices the kernel returned."""
    x, emb = _vq_wide.ragged_problem()
    n, d, h, w = x.shape
    k = emb.shape[0]
    m = _quantizer(k, d, False, emb)
    xg = x.to(DEV).requires_grad_(True)
    g = torch.Generator().manual_seed(8)
    up = torch.randn(x.shape, generator=g)
    st, loss = m(xg)
    ((st * up.to(DEV)).sum() + 1.7 * loss).backward()
    idx = m.last_indices.cpu().long()
    assert idx.shape == (n * h * w,) and int(idx.min()) >= 0 and int(idx.max()) < k
    dist, scale = _vq_wide.distances64(x, emb)
    best = dist.min(1).values
    mine = dist.gather(1, idx[:, None])[:, 0]
    excess = float(((mine - best) / scale).max())
    differ = int((idx != dist.argmin(1)).sum())
    print(f"[vq] worst accepted gap {excess:.3e} of the margin {_vq_wide.TIE_MARGIN:.0e}; {differ} of {idx.numel()} differ")
    assert excess <= _vq_wide.TIE_MARGIN, f"an index {excess:.3e} (relative) away from the nearest code"
    assert differ <= idx.numel() // 100, f"{differ} positions differ from the float64 argmin"
    # float64 restatement from the kernel's own indices
    x64, e64 = x.double(), emb.double()
    q64 = e64[idx].view(n, h, w, d).permute(0, 3, 1, 2)
    assert torch.equal(st.detach().cpu(), x + (emb[idx].view(n, h, w, d).permute(0, 3, 1, 2) - x))
    numel = x.numel()
    _util.assert_close(loss, 2 * ((x64 - q64) ** 2).mean(), 1e-5, "loss")
    want_dx = up.double() + 1.7 * 2 * (x64 - q64) / numel
    diff = (q64 - x64).permute(0, 2, 3, 1).reshape(-1, d)
    want_de = torch.zeros(k, d, dtype=torch.float64).index_add_(0, idx, diff) * (1.7 * 2 / numel)
    rep = _util.GradReport("vq ragged 11x130x10x10 K=300")
    rep.add("dx", xg.grad, want_dx)
    rep.add("d_embedding", m._embedding.grad, want_de)
    rep.finish()


@pytest.mark.parametrize("d,k,shape", [(8, 12, (3, 8, 5, 6)), (130, 300, (11, 130, 10, 10)), (64, 512, (32, 64, 8, 8))])
def test_codebook_gradient_is_bit_reproducible_and_fills_the_sink(d, k, shape):
    from pytorch_generative_amd import ops, optim

    g = torch.Generator().manual_seed(d * 131 + k)
    x = torch.randn(shape, generator=g).to(DEV)
    torch.manual_seed(d)
    base = _quantizer(k, d, False)
    runs = []
    prev = ops.set_deterministic(False)
    try:
        for det in (False, False, True, True):
            ops.set_deterministic(det)
            m = copy.deepcopy(base)
            xg = x.clone().requires_grad_(True)
            q, loss = m(xg)
            (q.sum() * 0.5 + 3.0 * loss).backward()
            runs.append((m._embedding.grad.clone(), xg.grad.clone()))
    finally:
        ops.set_deterministic(prev)
    for de, dx in runs[1:]:
        assert torch.equal(de, runs[0][0]), "d_embedding differs run to run"
        assert torch.equal(dx, runs[0][1])
    assert float(runs[0][0].abs().max()) > 0
    # through the flat-gradient sink: accumulated into FlatAdam's buffer, equal to the returned gradient
    m = copy.deepcopy(base)
    opt = optim.FlatAdam(m.parameters(), lr=1e-3)
    opt.zero_grad()
    q, loss = m(x.clone().requires_grad_(True))
    (q.sum() * 0.5 + 3.0 * loss).backward()
    assert m._embedding.grad is m._embedding._pg_grad
    assert torch.equal(m._embedding._pg_grad, runs[0][0])
    q, loss = m(x)  # a second backward adds
    (3.0 * loss).backward()
    assert torch.equal(m._embedding._pg_grad, runs[0][0] + runs[0][0])


def _sgd_vq_vae(seed=0):
    import pytorch_generative_amd as pg

    torch.manual_seed(seed)
    model = pg.models.VectorQuantizedVAE(in_channels=3, out_channels=3, hidden_channels=16, n_residual_blocks=1,
                                         residual_channels=8, n_embeddings=10, embedding_dim=80)
    model._quantizer._net[1] = pg.nn.VectorQuantizer(10, 80, use_ema=False)
    return model.to(DEV)


def test_graphed_steps_equal_eager_bitwise():
    from pytorch_generative_amd import graph, optim
    from pytorch_generative_amd.nn import utils as vq

    loss_fn = lambda x, preds: vq.mse_loss(preds[0], x) + preds[1]  # noqa: E731
    g = torch.Generator().manual_seed(5)
    xs = [torch.rand(2, 3, 16, 16, generator=g).to(DEV) for _ in range(4)]
    m1 = _sgd_vq_vae()
    m2 = copy.deepcopy(m1)
    o1, o2 = optim.FlatAdam(m1.parameters(), lr=1e-3), optim.FlatAdam(m2.parameters(), lr=1e-3)
    before = m1._quantizer._net[1]._embedding.detach().clone()
    for x in xs:
        o1.zero_grad()
        loss_fn(x, m1(x)).backward()
        o1.step()
    step = graph.GraphedTrainStep(m2, o2, loss_fn, xs[0], preserve_state=True)
    for x in xs:
        step(x)
    torch.cuda.synchronize()
    assert not torch.equal(m1._quantizer._net[1]._embedding, before), "the codebook must train"
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(p1, p2), f"{k}: graph replay differs from eager steps"
    for (k, b1), (_, b2) in zip(m1.named_buffers(), m2.named_buffers()):
        assert torch.equal(b1, b2), k


def test_wide_vq_vae_matches_reference_golden():
    """embedding_dim = 80, checked as test_gpu_f4.py checks vq_vae_small.pt."""
    import pytorch_generative_amd as pg
    from pytorch_generative_amd.nn import utils as vq

    g = _vq_wide.load_model()
    model = getattr(pg.models, g["ctor"])(**g["kwargs"]).to(DEV)
    model.load_state_dict(g["state0"])
    model.train()
    x = g["x"].to(DEV)
    recon, vq_loss = model(x)
    loss = vq.mse_loss(recon, x) + vq_loss
    loss.backward()
    _util.assert_close(recon, g["recon"], 1e-4, "reconstruction")
    _util.assert_close(vq_loss, g["vq_loss"], 1e-4, "quantization loss")
    _util.assert_close(loss, g["loss"], 1e-4, "loss")
    for k, p in model.named_parameters():
        want = g["grads"][k]
        if want is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
        else:
            _util.assert_close(p.grad, want, 1e-3, f"grad {k}")
    after = g["state_after_forward"]
    for k, v in model.state_dict().items():
        if k.endswith(("_embedding", "_cluster_size", "_embedding_avg")):
            _util.assert_close(v, after[k], 1e-5, f"buffer {k} after forward")
