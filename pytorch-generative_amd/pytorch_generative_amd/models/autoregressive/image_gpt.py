"""ImageGPT on the MI355X operator path.

Same constructor, attribute names (= state_dict keys) and forward graph as the reference's
models/autoregressive/image_gpt.py:21-109 — including its doubled residual (the block returns
x + ..., and the model loop adds x again, :50-52 vs :107-108) — with every op on HIP kernels:
NCHW LayerNorm, 1x1 convs (residual adds fused into the projection / MLP-out kernels), exact
GELU, and the fused causal attention core.
"""

import itertools

import torch
from torch import nn

from pytorch_generative_amd import _lib
from pytorch_generative_amd import graph as pg_graph
from pytorch_generative_amd import nn as pg_nn
from pytorch_generative_amd import ops
from pytorch_generative_amd.models import base


class TransformerBlock(nn.Module):
    def __init__(self, n_channels, n_attention_heads):
        super().__init__()
        self._ln1 = pg_nn.NCHWLayerNorm(n_channels)
        self._ln2 = pg_nn.NCHWLayerNorm(n_channels)
        self._attn = pg_nn.CausalAttention(
            in_channels=n_channels,
            n_heads=n_attention_heads,
            embed_channels=n_channels,
            out_channels=n_channels,
        )
        self._out = nn.Sequential(
            pg_nn.Conv2d(in_channels=n_channels, out_channels=4 * n_channels, kernel_size=1),
            nn.GELU(),  # placeholder keeping the Sequential indices; fused into _out[2]'s load
            pg_nn.Conv2d(in_channels=4 * n_channels, out_channels=n_channels, kernel_size=1),
        )

    def _fused_ok(self, x):
        return ops.gpt_block_supported(x, self._ln1, self._attn._q, self._attn._kv, self._attn._proj,
                                       self._ln2, self._out[0], self._out[2])

    def forward_plus_input(self, x):
        """x + self(x) — what the model loop computes (reference image_gpt.py:107) — on the fused
        head / attention / tail kernels (gpt_block.hip, ops.gpt_blocks) when the block has the BASELINE shape."""
        return ops.gpt_blocks(x, [self]) if self._fused_ok(x) else ops.add(x, self.forward(x))

    def forward(self, x):
        # skip=True: the residual branch's gradient is added inside the LayerNorm backward kernel
        y, x = self._ln1(x, skip=True)
        x = self._attn(y, res=x)                         # x + attn(ln1(x))
        y, x = self._ln2(x, skip=True)
        if ops.mlp_gelu_supported(y, self._out[0], self._out[2]):
            # fc1 -> GELU -> fc2 -> + x in one kernel each way: the hidden tensor stays in registers
            return ops.mlp_gelu(y, self._out[0], self._out[2], res=x)
        hidden = self._out[0](y)
        # exact GELU fused into the MLP-out kernel's input load, residual into its epilogue
        return self._out[2](hidden, in_act="gelu", res=x)  # x + mlp(ln2(x))


class ImageGPT(base.AutoregressiveModel):
    def __init__(
        self,
        in_channels=1,
        out_channels=1,
        in_size=28,
        n_transformer_blocks=8,
        n_attention_heads=4,
        n_embedding_channels=16,
        sample_fn=None,
    ):
        super().__init__(sample_fn)
        self._pos = nn.Parameter(torch.zeros(1, in_channels, in_size, in_size))
        self._input = pg_nn.CausalConv2d(
            mask_center=True,
            in_channels=in_channels,
            out_channels=n_embedding_channels,
            kernel_size=3,
            padding=1,
        )
        self._transformer = nn.ModuleList(
            TransformerBlock(n_channels=n_embedding_channels, n_attention_heads=n_attention_heads)
            for _ in range(n_transformer_blocks)
        )
        self._ln = pg_nn.NCHWLayerNorm(n_embedding_channels)
        self._out = pg_nn.Conv2d(
            in_channels=n_embedding_channels, out_channels=out_channels, kernel_size=1
        )

    _accepts_condition = True  # AutoregressiveModel.set_condition: a coarser code image as context (nn.CodeUpsample)

    def _check_cond(self, cond, hw):
        """The condition module for `cond` (None for neither); a ValueError when only one of the two is there or when the
        sizes do not match the (H, W) image."""
        mod = getattr(self, "_cond", None)
        if cond is None and mod is None:
            return None
        if mod is None:
            raise ValueError("ImageGPT: `cond` given, but the model has no condition module (set_condition)")
        if cond is None:
            raise ValueError("ImageGPT: the model has a condition module and needs `cond`")
        if self.input_codes is None:
            raise ValueError("ImageGPT: a condition module needs input_codes")
        f = mod.factor
        if cond.dim() != 4 or cond.shape[1] != 1 or (cond.shape[2] * f, cond.shape[3] * f) != tuple(hw):
            raise ValueError(f"ImageGPT: cond {tuple(cond.shape)} times the factor {f} is not the image size {tuple(hw)}")
        return mod

    # ---- code-index input (AutoregressiveModel.input_codes) ------------------------------------
    def _position_term(self):
        """W * _pos without the bias, (1, C, H, W): the data-independent half of _input(onehot + _pos) (the convolution is
        linear), on the dense kernels at batch 1; its gradient reaches _pos and the weight through them. The caller has
        masked the weight."""
        conv = self._input
        return ops.conv2d_taps(self._pos, conv.weight, None, conv._conv_spec(), weight_param=conv.weight)

    def _stem_codes(self, levels, cond=None):
        """_input(one_hot(codes) + _pos) for a code image (N, 1, H, W): lookup with the bias + the position term; with a
        condition module, + its lookup of `cond` in the same pass that copies the stem (ops.code_upsample)."""
        mod = self._check_cond(cond, levels.shape[2:])
        x = self._input.forward_codes(levels, self.input_codes)  # masks the weight in place first
        x = ops.add_broadcast_batch(x, self._position_term())
        if mod is None:
            return x
        if torch.is_grad_enabled():
            return mod(cond, base=x)
        return ops.code_upsample_(x, cond, mod.weight, mod.factor)  # x is this call's own tensor: added in place

    # ---- incremental sampling -------------------------------------------------
    def _decode_route(self, n):
        """Which block kernels the K/V-cached sampler runs for n samples: "blocks" — the fused head / tail block kernels with
        pg_attn_decode between them (the BASELINE shape: 16 channels, 64 hidden units), "step" — all blocks of a position in
        one launch (ops.gpt_decode_step: any width the planner accepts), None — no cached route (a full forward per pixel)."""
        if self._input.bias is None:
            return None
        ld = (n + 15) // 16 * 16
        probe = torch.empty(1, self._input.weight.shape[0], 1, ld, device="meta")
        if all(blk._fused_ok(probe) for blk in self._transformer):
            return "blocks"
        return "step" if ops.gpt_decode_supported(self) else None

    def _incremental_ok(self, n):
        return self._decode_route(n) is not None

    @base.dense_head
    @torch.no_grad()
    def sample(self, n_samples=None, conditioned_on=None, *, cond=None, incremental=True, return_logits=False, route=None):
        """Same contract as the reference's AutoregressiveModel.sample (models/base.py:97-120: raster
        order, only entries < 0 are drawn, `_sample_fn` called once per pixel on (n, c) logits) — but
        each step evaluates ONLY the current position: the model is causal, so the activations of
        pixel p are final once pixels < p are. One position of all samples is a (channels, batch)
        matrix, i.e. the (C, L) plane layout of the block kernels with the batch as the pixel axis:
        the fused head / tail kernels run unchanged, attention becomes a one-query-per-(n, head)
        decode against per-layer K / V caches. At any other width the planner accepts, ONE launch per
        position carries every sample through all blocks (ops.gpt_decode_step, `_decode_route`). The
        reference (and `incremental=False`) instead runs one full forward per pixel: H*W times the work.

        cond (extension): the coarser code image (n, 1, H / f, W / f) of a model with a condition module (set_condition); n
        comes from it when neither n_samples nor conditioned_on is given. Every route honours it.
        return_logits (extension): also returns the (H*W, n, c) logits the draws were made from.
        route (measurement aid, tools/gpt_decode_bench.py): "step" runs the one-launch step kernel on a model that would
        take the block kernels. The route that ran is left in `_sample_route` ("blocks", "step" or "full")."""
        if n_samples is None and conditioned_on is None and cond is not None:
            n_samples = cond.shape[0]
        canvas = self._start_canvas(n_samples, conditioned_on)
        n, c, h, w = canvas.shape
        cond_mod = self._check_cond(cond, (h, w))
        if cond_mod is not None:
            if cond.shape[0] != n:
                raise ValueError(f"sample: cond holds {cond.shape[0]} images, the canvas {n}")
            cond = cond.to(canvas.device).contiguous()
        decode = self._decode_route(n) if incremental else None
        if route is not None and decode is not None:
            if route not in ("blocks", "step") or (route == "blocks" and decode != "blocks"):
                raise ValueError(f"sample: route {route!r} is not available for this model")
            if route == "step" and not ops.gpt_decode_supported(self):
                raise ValueError("sample: the step kernel does not cover this model")
            decode = route
        self._sample_route = decode or "full"
        if decode is None:
            if return_logits:
                raise ValueError("return_logits needs the incremental sampler")
            if cond_mod is None:
                return super().sample(conditioned_on=canvas)
            for row in range(h):  # the reference's loop (models/base.py:97-120) with the context passed to every forward
                for col in range(w):
                    self._draw_into(canvas, row, col, self.forward(canvas, cond)[:, :, row, col])
            return canvas
        lib = _lib.load()
        dev, L = canvas.device, h * w
        canvas = canvas.contiguous()
        ld = (n + 15) // 16 * 16
        conv = self._input
        emb = conv.weight.shape[0]
        kh, kw = conv.weight.shape[2], conv.weight.shape[3]
        ops.mul_inplace_(conv.weight.data, conv.mask)  # nn/convolution.py:42, as on every forward
        blocks = list(self._transformer)
        attn0 = blocks[0]._attn
        k_cache = torch.zeros(len(blocks), n, attn0._embed_channels, L, device=dev)
        v_cache = torch.zeros(len(blocks), n, attn0._out_channels, L, device=dev)
        pack = ops.gpt_decode_pack(blocks) if decode == "step" else None  # once per call
        x = torch.zeros(1, emb, 1, ld, device=dev)
        pos_dev = torch.zeros(1, dtype=torch.int32, device=dev)  # raster position, advanced on the device

        n_codes = self.input_codes
        if n_codes is not None:
            if c != 1 or int(n_codes) != conv.in_channels or (h, w) != tuple(self._pos.shape[2:]):
                raise ValueError(f"sample: input_codes = {n_codes} needs a (N, 1, {self._pos.shape[2]}, {self._pos.shape[3]}) "
                                 f"canvas and {n_codes} stem input channels")
            pos_term = self._position_term().contiguous()  # once per call

        def position_logits():
            """logits (n, c) of the position in pos_dev; appends its keys / values to the caches"""
            st = torch.cuda.current_stream().cuda_stream
            if n_codes is not None:
                _lib.check(lib.pg_sample_embed_codes(canvas.data_ptr(), conv.weight.data_ptr(), conv.bias.data_ptr(),
                                                     pos_term.data_ptr(), x.data_ptr(), n, int(n_codes), h, w, emb, kh, kw,
                                                     0, 0, ld, pos_dev.data_ptr(), st), "pg_sample_embed_codes")
            else:
                _lib.check(lib.pg_sample_embed(canvas.data_ptr(), self._pos.data_ptr(),
                                               conv.weight.data_ptr(), conv.bias.data_ptr(), x.data_ptr(),
                                               n, c, h, w, emb, kh, kw, 0, 0, ld, pos_dev.data_ptr(), st),
                           "pg_sample_embed")
            if cond_mod is not None:
                cond_mod.add_position_(x, cond, pos_dev, ld)
            if decode == "step":  # every block of the position in one launch, in place
                cur = ops.gpt_decode_step(x, pack, k_cache, v_cache, pos_dev, heads=attn0._n_heads,
                                          strict=int(attn0._mask_center), eps=blocks[0]._ln1.eps)
            else:
                cur = x
                for blk, kc, vc in zip(blocks, k_cache, v_cache):
                    a = blk._attn
                    qkv, xs = ops.gpt_block_head(cur, blk._ln1, a._q, a._kv)
                    o = torch.empty(1, a._out_channels, 1, ld, device=dev)
                    _lib.check(lib.pg_attn_decode(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                                                  o.data_ptr(), n, a._n_heads, L, 0,
                                                  a._embed_channels // a._n_heads,
                                                  a._out_channels // a._n_heads, ld, int(a._mask_center),
                                                  pos_dev.data_ptr(), st), "pg_attn_decode")
                    cur = ops.gpt_block_tail(o, xs, a._proj, blk._ln2, blk._out[0], blk._out[2])
            return self._out(self._ln(cur))[0, :, 0, :n].t().contiguous()

        def step():
            logits = position_logits()
            pos_dev.add_(1)
            return logits

        # One hipGraph = one position of every layer (~30 launches; a handful on the step kernel) + the position increment; only the
        # draw (`_sample_fn` is user code) and the canvas update stay eager. Falls back to eager
        # launches if the capture is refused. (The warm-up at position 0 rewrites cache column 0 with the same values.)
        pairs = pg_graph.try_capture([step], position_logits)
        graph, static_logits = pairs[0] if pairs else (None, None)
        pos_dev.zero_()
        all_logits = []
        for row in range(h):
            for col in range(w):
                if graph is not None:
                    graph.replay()
                    logits = static_logits.clone() if return_logits else static_logits
                else:
                    logits = step()
                if return_logits:
                    all_logits.append(logits)
                self._draw_into(canvas, row, col, logits)
        if return_logits:
            return canvas, torch.stack(all_logits)
        return canvas

    def forward(self, x, cond=None):
        img, blocks, grad = x, list(self._transformer), torch.is_grad_enabled()
        # the two ends on their own kernels (gpt_ends.hip) where the model has the BASELINE shape; PG_FUSE_ENDS=0 = generic operators
        codes = self.input_codes is not None  # the stem as a table lookup: the fused stem is not taken
        if not codes:
            self._check_cond(cond, img.shape[2:])  # a cond or a condition module without input_codes raises
        fuse_stem = not codes and ops.gpt_stem_supported(img, self._pos, self._input)
        # The stem's backward runs last: a trainable fused stem flushes the chain on its only path, whichever blocks queued rows
        stem_flushes = fuse_stem and grad and any(p.requires_grad for p in (self._pos, self._input.weight, self._input.bias))
        if fuse_stem:
            x0_grad = stem_flushes
            probe = torch.empty(1, self._input.weight.shape[0], img.shape[2], img.shape[3], device="meta")
        elif codes:
            x = probe = self._stem_codes(img, cond)
            x0_grad = x.requires_grad
        else:
            x = probe = self._input(ops.add_broadcast_batch(img, self._pos))
            x0_grad = x.requires_grad
        # one queue for the weight-gradient partial rows of the blocks (and of the output head) — only when every block takes the
        # fused kernels and a backward pass with a gradient for the first block's input will run. Without a flushing stem the
        # FIRST block flushes (its backward runs last among the blocks); it queues only on its all-sinks path, so the chain is
        # then declined unless every block parameter has a sink.
        chain = None
        if (grad and x0_grad and len(blocks) > 1 and all(b._fused_ok(probe) for b in blocks)
                and (stem_flushes or all(ops._sink(p) is not None for b in blocks for p in b.parameters()))):
            chain = ops.new_block_chain()
        if fuse_stem:
            x = self._input(img, pos=self._pos, chain=chain if stem_flushes else None)
        # every maximal run of blocks that take the fused kernels (all of them or none, in practice) is one autograd node, which
        # runs each boundary inside it — tail(i) + head(i+1), and head(i+1) + tail(i) backward — as one launch (ops.gpt_blocks)
        for ok, run in itertools.groupby(blocks, key=lambda b: b._fused_ok(probe)):
            run = list(run)
            if ok:
                x = ops.gpt_blocks(x, run, chain, flush=run[0] is blocks[0] and not stem_flushes)
            else:
                for block in run:
                    x = block.forward_plus_input(x)
        # defer_head: the head runs inside the loss (ops.DeferredLogits) and reduces its own rows: it does not join the chain
        return self._logits(x, self._out, pre_ln=self._ln, chain=chain if stem_flushes else None)


def reproduce(n_epochs=457, batch_size=64, log_dir="/tmp/run", n_gpus=1, device_id=0,
              debug_loader=None):
    """The reference's training recipe for this model (image_gpt.py:112-175: same model
    hyper-parameters, Adam lr 5e-3, per-batch lr decay 0.999977) on the MI355X path. Arguments as the reference;
    `debug_loader` replaces both loaders (any iterable of (x, y) batches). Returns the Trainer."""
    from pytorch_generative_amd import recipes

    return recipes.run(
        lambda: ImageGPT(in_channels=1, out_channels=1, in_size=28, n_transformer_blocks=8,
                         n_attention_heads=2, n_embedding_channels=64),
        loaders=recipes.binarized_mnist, loss_fn=recipes.bce_loss, lr=5e-3, lr_decay=0.999977,
        n_epochs=n_epochs, batch_size=batch_size, log_dir=log_dir, n_gpus=n_gpus,
        device_id=device_id, debug_loader=debug_loader)
