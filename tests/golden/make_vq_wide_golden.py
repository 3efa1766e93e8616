"""Generates tests/golden/vq_wide/ from the REAL reference (run in the build container only):

    python tests/golden/make_vq_wide_golden.py

VectorQuantizer (nn/utils.py:16-96) at embedding widths above 64 and in BOTH codebook modes — the EMA buffers and the
codebook trained by gradient descent — plus one small VectorQuantizedVAE with embedding_dim=80.

Per case one forward and one backward of `q.sum() * 0.5 + loss`, as make_vq_golden.py does, with the same codebook and the
same input in both modes (the quantized output, dx and the indices are then the same tensors: asserted, stored once).
Files (a committed file stays below 1 MiB, and the largest case alone is larger than that, so there is one pair per case):
  cases.pt            the list of case names and the tie margin
  <case>.pt           x, the codebook, indices, quantized, dx, both losses, d_embedding of the gradient mode
  <case>_ema.pt       the EMA mode's buffers before (`_cluster_size`, `_embedding_avg`) and after the training forward
  vq_vae_wide.pt      the model, stored as vq_vae_small.pt is

Tie margin: a seed is kept only if for every position, in float64,
    second-best distance - best distance >= TIE_MARGIN * (|x|^2 + max_k |e_k|^2)
(about 100 times the fp32 round-off of a 200-term distance), so the indices of any correct fp32 evaluation are THE indices
and can be compared exactly; otherwise the next salt is tried. The duplicate-row case measures the gap to the third-best
distance: its two best are the identical rows, and the lower index must win.
"""

import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _ref  # noqa: E402

OUT = os.path.join(HERE, "vq_wide")
TIE_MARGIN = 1e-4
SALTS = 2000  # the 513-code case passes about one seed in a hundred

# name -> (D, K, x shape, duplicate rows (kept, copy) or None)
CASES = {
    "d65_k7": (65, 7, (2, 65, 5, 9), None),        # first width past the old limit; ragged D chunk; K below one tile
    "d96_k33": (96, 33, (3, 96, 6, 7), None),      # K one past a tile; P not a tile multiple
    "d128_k513": (128, 513, (3, 128, 7, 9), None),  # several code tiles; the last tile holds one code
    "d200_k130": (200, 130, (1, 200, 6, 10), None),  # D not a multiple of 16; N = 1
    "d70_k1": (70, 1, (2, 70, 3, 3), None),        # a single code; P = 18
    "d72_k9_dup": (72, 9, (2, 72, 4, 5), (2, 6)),  # rows 2 and 6 identical: 2 must win
}


def tie_gap(flat_x, emb, skip=1):
    """min over positions of (the (skip+1)-th smallest distance - the smallest) / (|x|^2 + max |e|^2), in float64;
    +inf when there are not that many codes."""
    x, e = flat_x.double(), emb.double()
    dist = (x * x).sum(1, keepdim=True) + (e * e).sum(1) - 2 * x @ e.t()
    if dist.shape[1] <= skip:
        return float("inf"), dist.argmin(1)
    srt = dist.sort(dim=1).values
    scale = (x * x).sum(1) + (e * e).sum(1).max()
    return float(((srt[:, skip] - srt[:, 0]) / scale).min()), dist.argmin(1)


def flat(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def run(ref, emb, x, use_ema, ema_state=None):
    d = emb.shape[1]
    vq = ref.nn.VectorQuantizer(n_embeddings=emb.shape[0], embedding_dim=d, use_ema=use_ema)
    with torch.no_grad():
        vq._embedding.copy_(emb)
        if use_ema:
            vq._cluster_size.copy_(ema_state["_cluster_size"])
            vq._embedding_avg.copy_(ema_state["_embedding_avg"])
    vq.train()
    before = _ref.clone_state(vq)
    xin = x.clone().requires_grad_(True)
    q, loss = vq(xin)
    (q.sum() * 0.5 + loss).backward()
    return {"before": before, "quantized": q.detach().clone(), "loss": loss.detach().clone(),
            "dx": xin.grad.detach().clone(), "after": _ref.clone_state(vq),
            "d_embedding": None if use_ema else vq._embedding.grad.detach().clone()}


def make_case(ref, name, spec, base_seed):
    d, k, shape, dup = spec
    for salt in range(SALTS):
        torch.manual_seed(base_seed + 1000 * salt)
        emb = ref.nn.VectorQuantizer(n_embeddings=k, embedding_dim=d, use_ema=False)._embedding.detach().clone()
        if dup:
            emb[dup[1]] = emb[dup[0]]
        x = torch.randn(*shape)
        gap, idx64 = tie_gap(flat(x), emb, skip=2 if dup else 1)
        if gap < TIE_MARGIN:
            continue
        if dup and not bool((idx64 == dup[0]).any()):
            continue  # the duplicated row must be somebody's nearest code, or the case shows nothing
        break
    else:
        raise RuntimeError(f"{name}: no seed in {SALTS} salts satisfies the tie margin")
    cs = torch.empty(k).uniform_(0.5, 4.0)  # a used codebook: non-trivial cluster sizes / averages
    ema_state = {"_cluster_size": cs, "_embedding_avg": emb * cs.unsqueeze(1)}
    sgd = run(ref, emb, x, False)
    ema = run(ref, emb, x, True, ema_state)
    # float64's nearest code is the reference's, and both modes quantize alike
    n, _, h, w = shape
    want_q = emb[idx64].view(n, h, w, d).permute(0, 3, 1, 2).contiguous()
    want_q = x + (want_q - x)  # the straight-through value the module returns (:95)
    assert torch.equal(sgd["quantized"], want_q) and torch.equal(ema["quantized"], want_q), name
    assert torch.equal(sgd["dx"], ema["dx"]), name
    assert list(sgd["before"]) == ["_embedding"] and torch.equal(sgd["after"]["_embedding"], emb), name
    if dup:
        assert not bool((idx64 == dup[1]).any()), name
    main = {"embedding_dim": d, "n_embeddings": k, "x": x, "embedding": emb, "indices": idx64.to(torch.int32),
            "quantized": sgd["quantized"], "dx": sgd["dx"], "loss_sgd": sgd["loss"], "loss_ema": ema["loss"],
            "d_embedding": sgd["d_embedding"], "duplicate_rows": dup, "tie_gap": gap, "salt": salt,
            "torch_version": torch.__version__}
    ema_rec = {"before": {key: ema["before"][key] for key in ("_cluster_size", "_embedding_avg")}, "after": ema["after"]}
    for fname, rec in ((name + ".pt", main), (name + "_ema.pt", ema_rec)):
        path = os.path.join(OUT, fname)
        torch.save(rec, path)
        size = os.path.getsize(path)
        assert size < (1 << 20), f"{fname}: {size} bytes"
        print(f"{fname}: {size / 1024:.0f} KiB (salt {salt}, gap {gap:.2e})")


def make_model(ref):
    import torch.nn.functional as F

    kwargs = dict(in_channels=3, out_channels=3, hidden_channels=16, n_residual_blocks=1, residual_channels=8,
                  n_embeddings=10, embedding_dim=80)
    x = torch.randint(0, 256, (2, 3, 16, 16), generator=torch.Generator().manual_seed(1234)).float() / 255
    for salt in range(SALTS):
        torch.manual_seed(salt)
        model = ref.models.VectorQuantizedVAE(**kwargs)
        model.train()
        state0 = _ref.clone_state(model)
        seen = {}
        vqs = [m for m in model.modules() if isinstance(m, ref.nn.VectorQuantizer)]
        assert len(vqs) == 1
        hook = vqs[0].register_forward_pre_hook(
            lambda m, inp: seen.update(x=inp[0].detach().clone(), e=m._embedding.detach().clone()))
        opt = torch.optim.Adam(model.parameters(), lr=2e-4)
        opt.zero_grad()
        recon, vq_loss = model(x)
        hook.remove()
        gap, _ = tie_gap(flat(seen["x"]), seen["e"])
        if gap >= TIE_MARGIN:
            break
    else:
        raise RuntimeError(f"vq_vae_wide: no seed in {SALTS} salts satisfies the tie margin")
    loss = F.mse_loss(recon, x) + vq_loss
    loss.backward()
    state_fwd = _ref.clone_state(model)
    norm = torch.nn.utils.clip_grad_norm_(model.parameters(), 1e50)
    grads = {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in model.named_parameters()}
    opt.step()
    rec = {"ctor": "VectorQuantizedVAE", "kwargs": kwargs, "lr": 2e-4, "x": x, "state0": state0,
           "recon": recon.detach().clone(), "vq_loss": vq_loss.detach().clone(), "loss": loss.detach().clone(),
           "grads": grads, "grad_norm": norm.detach().clone(), "state_after_forward": state_fwd,
           "state1": _ref.clone_state(model), "quantizer_input": seen["x"], "tie_gap": gap, "salt": salt,
           "torch_version": torch.__version__}
    path = os.path.join(OUT, "vq_vae_wide.pt")
    torch.save(rec, path)
    assert os.path.getsize(path) < (1 << 20)
    print(f"vq_vae_wide: loss={float(loss.detach()):.6f} vq={float(vq_loss.detach()):.6f} salt {salt} gap {gap:.2e} "
          f"-> {os.path.getsize(path) / 1024:.0f} KiB")


def main():
    ref = _ref.load()
    os.makedirs(OUT, exist_ok=True)
    for i, (name, spec) in enumerate(CASES.items()):
        make_case(ref, name, spec, 17 + i)
    make_model(ref)
    torch.save({"cases": list(CASES), "tie_margin": TIE_MARGIN, "model": "vq_vae_wide",
                "torch_version": torch.__version__}, os.path.join(OUT, "cases.pt"))


if __name__ == "__main__":
    main()
