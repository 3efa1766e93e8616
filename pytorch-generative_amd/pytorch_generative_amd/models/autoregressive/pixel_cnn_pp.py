"""PixelCNN++ on the MI355X operator path — SURVEY.md §8(f) rank 4 (BASELINE.json configs[2] names it).

The reference repository has NO PixelCNN++; this module follows the published architecture — Salimans,
Karpathy, Chen, Kingma, "PixelCNN++", ICLR 2017 (section 2: discretized logistic mixture likelihood,
conditioning on whole pixels, two streams of down-shifted / down-right-shifted convolutions, gated
residual blocks on concatenated ELUs, down- and up-sampling by strided convolutions with short-cut
connections across the three resolutions). Its CPU restatement is oracle/pixelcnnpp.py, written on
torch's strided / transposed convolutions; since there is no reference implementation, parity means HIP
path == that oracle plus the autoregressive property (tests/test_gpu_f4.py, tests/test_dmol_cpu.py).

How the pieces map onto this package's kernels:
  * down-shifted (2 x 3) and down-right-shifted (2 x 2) convolutions, and the extra row / column shift
    of the input layers, are tap lists of the masked-convolution kernels (padding + crop, no shifting
    copies);
  * stride-2 down-sampling = the stride-1 shifted convolution followed by ops.subsample2; stride-2
    up-sampling = ops.zero_insert2 followed by the same shifted convolution (the transposed convolution
    of the paper written as a gather);
  * the gate a * sigmoid(b) + residual is GatedActivation's fused kernel; concat_elu is ops.concat_elu;
  * the loss is ops.dmol_loss_sum_mean on images scaled to [-1, 1].
"""

import torch
from torch import nn

from pytorch_generative_amd import _lib
from pytorch_generative_amd import nn as pg_nn
from pytorch_generative_amd import ops
from pytorch_generative_amd.models import base


class ShiftedConv2d(pg_nn.Conv2d):
    """kind "ds": down-shifted — the (kh x kw) window ends at the output's row and is centred on its
    column; kind "drs": down-right-shifted — the window ends at the output's row AND column.
    shift_down / shift_right move the whole window one more row up / column left (the input layers)."""

    def __init__(self, in_channels, out_channels, kernel_size, kind, shift_down=False, shift_right=False):
        kh, kw = kernel_size
        assert kind in ("ds", "drs") and (kind == "drs" or kw % 2 == 1)
        ph = kh - 1 + int(shift_down)
        pw = (kw - 1 if kind == "drs" else (kw - 1) // 2) + int(shift_right)
        super().__init__(in_channels, out_channels, kernel_size=(kh, kw), padding=(ph, pw))

    def forward(self, x, **kw):
        return super().forward(x, crop=(x.shape[2], x.shape[3]), **kw)


class GatedResnet(nn.Module):
    """x + a' * sigmoid(b'), [a' | b'] = conv2(concat_elu(conv1(concat_elu(x)) + nin(concat_elu(aux))))."""

    def __init__(self, n_filters, kind, aux_channels=0):
        super().__init__()
        ks = (2, 3) if kind == "ds" else (2, 2)
        self._conv_in = ShiftedConv2d(2 * n_filters, n_filters, ks, kind)
        self._nin = pg_nn.Conv2d(2 * aux_channels, n_filters, kernel_size=1) if aux_channels else None
        self._conv_out = ShiftedConv2d(2 * n_filters, 2 * n_filters, ks, kind)
        self._gate = pg_nn.GatedActivation(activation_fn=nn.Identity())

    def forward(self, x, aux=None):
        # x has two readers (the activation and the gate's residual): two pass-through aliases, whose gradients one launch sums
        # (ops.fanout) instead of autograd's add kernel
        x, x_res = ops.fanout(x, 2)
        c1 = self._conv_in(ops.concat_elu(x))
        if aux is not None:
            c1 = self._nin(ops.concat_elu(aux), res=c1)
        c2 = self._conv_out(ops.concat_elu(c1))
        return self._gate(c2, res=x_res)


def row_schedule(h):
    """Which resolution level is evaluated at which image row, for row-by-row evaluation of the three-level network:
    entry y is the tuple of (level, row of that level) pairs of image row y, finest level first. Level s (H / 2**s rows)
    is evaluated at image row y iff y % 2**s == 0, on its row y >> s: row r of a sub-sampled down convolution is row 2r
    of the stride-1 convolution (reading fine rows 2r - 1 and 2r), and row r of an up convolution reads rows r - 1 and r
    of the zero-inserted tensor, whose even rows 2q are coarse row q and whose odd rows are zeros."""
    h = int(h)
    if h <= 0 or h % 4:
        raise ValueError("row_schedule: H must be a positive multiple of 4 (two stride-2 levels)")
    return [tuple((s, y >> s) for s in range(3) if y % (1 << s) == 0) for y in range(h)]


class PixelCNNpp(base.AutoregressiveModel):
    """forward(x) -> (N, 10 * n_mix, H, W) mixture parameters for images x in [-1, 1] with 3 channels
    (H, W multiples of 4). Paper configuration: n_filters=160, n_resnet=5, n_mix=10."""

    def __init__(self, in_channels=3, n_filters=160, n_resnet=5, n_mix=10, sample_fn=None):
        super().__init__(sample_fn)
        self._pixel_sample_fn = sample_fn  # None: the mixture draw (ops.dmol_sample); else fn(params (N, 10 K)) -> (N, 3)
        if in_channels != 3:
            raise ValueError("PixelCNNpp: the discretized logistic mixture conditions R, G, B sub-pixels (3 channels)")
        f, cin = n_filters, in_channels + 1  # + a channel of ones (so that the shifted convolutions see the border)
        self._n_mix, self._n_resnet = n_mix, n_resnet
        self._u_in = ShiftedConv2d(cin, f, (2, 3), "ds", shift_down=True)
        self._ul_in_a = ShiftedConv2d(cin, f, (1, 3), "ds", shift_down=True)
        self._ul_in_b = ShiftedConv2d(cin, f, (2, 1), "drs", shift_right=True)
        self._up_u = nn.ModuleList([nn.ModuleList([GatedResnet(f, "ds") for _ in range(n_resnet)]) for _ in range(3)])
        self._up_ul = nn.ModuleList([nn.ModuleList([GatedResnet(f, "drs", aux_channels=f) for _ in range(n_resnet)])
                                     for _ in range(3)])
        self._down_u_conv = nn.ModuleList([ShiftedConv2d(f, f, (2, 3), "ds") for _ in range(2)])
        self._down_ul_conv = nn.ModuleList([ShiftedConv2d(f, f, (2, 2), "drs") for _ in range(2)])
        counts = [n_resnet, n_resnet + 1, n_resnet + 1]
        self._dn_u = nn.ModuleList([nn.ModuleList([GatedResnet(f, "ds", aux_channels=f) for _ in range(c)])
                                    for c in counts])
        self._dn_ul = nn.ModuleList([nn.ModuleList([GatedResnet(f, "drs", aux_channels=2 * f) for _ in range(c)])
                                     for c in counts])
        self._up_u_conv = nn.ModuleList([ShiftedConv2d(f, f, (2, 3), "ds") for _ in range(2)])
        self._up_ul_conv = nn.ModuleList([ShiftedConv2d(f, f, (2, 2), "drs") for _ in range(2)])
        self._out = pg_nn.Conv2d(f, 10 * n_mix, kernel_size=1)

    def forward(self, x):
        return self._net(x)

    def _net(self, x):
        """The network body on images in [-1, 1]. forward() and sample() both call THIS, so that a subclass whose
        forward() rescales its input (reproduce()'s wrapper for [0, 1] loaders) does not rescale the sampler's canvas."""
        self._no_input_codes()
        n, _, h, w = x.shape
        if h % 4 or w % 4:
            raise ValueError("PixelCNNpp: H and W must be multiples of 4 (two stride-2 levels)")
        xp = ops.concat_channels([x, torch.ones((n, 1, h, w), device=x.device, dtype=x.dtype)])
        # Every stream tensor of the up pass has two readers — the next layer and, later, the down pass's short-cut (a tensor
        # of the u stream a third one: the ul stream's layer of the same step): each reader takes its own pass-through alias
        # (ops.fanout), so that the gradients are summed by one launch per tensor instead of autograd's chains of add kernels.
        # `u_cur` / `ul_cur` = the alias for the next layer, u / ul = the stacks of short-cut aliases.
        u_cur, a = ops.fanout(self._u_in(xp), 2)
        ul_cur, b = ops.fanout(self._ul_in_b(xp, res=self._ul_in_a(xp)), 2)
        u, ul = [a], [b]
        for s in range(3):  # up pass: towards the coarse resolution
            for ru, rul in zip(self._up_u[s], self._up_ul[s]):
                u_cur, u_aux, a = ops.fanout(ru(u_cur), 3)
                ul_cur, b = ops.fanout(rul(ul_cur, aux=u_aux), 2)
                u.append(a)
                ul.append(b)
            if s < 2:
                u_cur, a = ops.fanout(ops.subsample2(self._down_u_conv[s](u_cur)), 2)
                ul_cur, b = ops.fanout(ops.subsample2(self._down_ul_conv[s](ul_cur)), 2)
                u.append(a)
                ul.append(b)
        hu, hul = u.pop(), ul.pop()  # (the last tensors' "next layer" aliases stay unused: they carry no gradient)
        for s in range(3):  # down pass: back to the fine resolution, short-cuts from the up pass
            for ru, rul in zip(self._dn_u[s], self._dn_ul[s]):
                hu, hu_cat = ops.fanout(ru(hu, aux=u.pop()), 2)  # read by the ul stream's concatenation and by the next layer
                hul = rul(hul, aux=ops.concat_channels([hu_cat, ul.pop()]))
            if s < 2:
                hu = self._up_u_conv[s](ops.zero_insert2(hu))
                hul = self._up_ul_conv[s](ops.zero_insert2(hul))
        assert not u and not ul
        return self._out(hul, in_act="elu")

    # ---- row-cached incremental sampling -----------------------------------------------------------------------------
    def _row_const(self, key, shape, value, device):
        """A constant (ones channel, rows of zeros) of the row step, filled once by the library's own kernel and never written."""
        cache = self.__dict__.setdefault("_row_consts", {})
        k = (key, tuple(shape), str(device))
        if k not in cache:
            t = torch.empty(shape, device=device, dtype=torch.float32)
            _lib.check(_lib.load().pg_fill(t.data_ptr(), float(value), t.numel(), ops._stream()), "pg_fill")
            cache[k] = t
        return cache[k]

    def _row_net(self, ctx, row_in):
        """_net on ONE image row under ops.RowDecode: row_in (N, 3, 1, W) is row ctx.row of an image in [-1, 1]; returns
        the (N, 10 K, 1, W) parameters of that row. The network is row-causal level by level (row_schedule): every
        convolution is a stride-1 shifted convolution with kh <= 2 whose band of earlier input rows nn.Conv2d keeps;
        sub-sampling keeps the even columns of the rows that survive it, zero insertion feeds a column-stuffed row at
        even rows of the finer level and a row of zeros at odd ones. Layers of a level that is not evaluated at this
        row are not called, so their bands do not move; a down convolution whose output row is dropped (odd rows of its
        input level) is called in the commit pass only, to push its band."""
        y = ctx.row
        deepest = row_schedule(ctx.height)[y][-1][0]
        n, _, _, w = row_in.shape
        dev = row_in.device
        xp = ops.concat_channels([row_in, self._row_const("ones", (n, 1, 1, w), 1.0, dev)])
        u_cur = self._u_in(xp)
        ul_cur = self._ul_in_b(xp, res=self._ul_in_a(xp))
        us, uls = [[u_cur]], [[ul_cur]]  # the short-cut stacks, one per evaluated level
        for s in range(deepest + 1):  # up pass
            for ru, rul in zip(self._up_u[s], self._up_ul[s]):
                u_cur = ru(u_cur)
                ul_cur = rul(ul_cur, aux=u_cur)
                us[s].append(u_cur)
                uls[s].append(ul_cur)
            if s < 2:
                used = s < deepest  # row y >> s of level s is even: it survives the sub-sampling
                if used or ctx.commit:
                    du, dul = self._down_u_conv[s](u_cur), self._down_ul_conv[s](ul_cur)
                if used:
                    u_cur, ul_cur = ops.col_subsample2(du), ops.col_subsample2(dul)
                    us.append([u_cur])
                    uls.append([ul_cur])
        hu = hul = None
        for s in range(3):  # down pass; _dn_*[s] live at level 2 - s
            lvl = 2 - s
            if lvl > deepest:
                continue
            if lvl == 2:
                hu, hul = us[2].pop(), uls[2].pop()
            else:
                if lvl < deepest:  # the coarser level was evaluated at this row: its row, zeros between the columns
                    zu, zul = ops.col_zero_insert2(hu), ops.col_zero_insert2(hul)
                else:              # an odd row of the zero-inserted tensor
                    zu = zul = self._row_const("zeros", (n, self._up_u_conv[s - 1].in_channels, 1, w >> lvl), 0.0, dev)
                hu, hul = self._up_u_conv[s - 1](zu), self._up_ul_conv[s - 1](zul)
            for ru, rul in zip(self._dn_u[s], self._dn_ul[s]):
                hu = ru(hu, aux=us[lvl].pop())
                hul = rul(hul, aux=ops.concat_channels([hu, uls[lvl].pop()]))
            assert not us[lvl] and not uls[lvl]
        return self._out(hul, in_act="elu")

    def _row_reset(self):
        self._row_consts = {}

    @staticmethod
    def sample_from_mixture(params, n_mix):
        """One draw per image from the discretized logistic mixture at ONE pixel: params (N, 10 K) in the channel
        layout of the loss (mixture logits, then per sub-pixel means / log-scales / coefficients) -> (N, 3) in
        [-1, 1]. The published sampler (Salimans et al. 2017, section 2.1-2.2 and the authors' implementation):
        component by the Gumbel-max trick, a logistic variate by inverse CDF, then G and B shifted by their
        linear dependence on the already drawn sub-pixels (eq. 3), each clamped to the image range."""
        n, k = params.shape[0], n_mix
        logits = params[:, :k]
        rest = params[:, k:].reshape(n, 3, 3 * k)
        u = torch.rand_like(logits).clamp_(1e-5, 1.0 - 1e-5)
        sel = torch.argmax(logits - torch.log(-torch.log(u)), dim=1)                       # (N,)
        pick = lambda t: t.gather(2, sel.view(n, 1, 1).expand(n, 3, 1)).squeeze(2)          # noqa: E731  (N, 3)
        means = pick(rest[:, :, :k])
        log_scales = pick(rest[:, :, k:2 * k]).clamp(min=-7.0)
        coeffs = torch.tanh(pick(rest[:, :, 2 * k:]))
        v = torch.rand_like(means).clamp_(1e-5, 1.0 - 1e-5)
        x = means + torch.exp(log_scales) * (torch.log(v) - torch.log1p(-v))
        x0 = x[:, 0].clamp(-1.0, 1.0)
        x1 = (x[:, 1] + coeffs[:, 0] * x0).clamp(-1.0, 1.0)
        x2 = (x[:, 2] + coeffs[:, 1] * x0 + coeffs[:, 2] * x1).clamp(-1.0, 1.0)
        return torch.stack((x0, x1, x2), dim=1)

    # Below this batch size sample() takes the full-forward procedure even when incremental=True (the rule of
    # base.AutoregressiveModel._row_decode_min_batch). The comparison that would set it is NOT YET MEASURED: one MI355X run
    # (profiles/pixelcnnpp_sampling.json) has the row-cached call at the paper configuration, 32 x 32, at 10.2 / 10.4 / 11.8 s
    # for n = 1 / 16 / 64, but no whole-call figure of the full-forward sampler to hold against it
    # (tools/pixelcnnpp_sample_bench.py measures both). Until it exists every batch size takes the row-cached path.
    _incremental_min_batch = 1
    _row_graph = True  # capture the row steps into hipGraphs (False: launch them eagerly; tools/pixelcnnpp_sample_bench.py)

    @torch.no_grad()
    def sample(self, n_samples=None, conditioned_on=None, *, image_size=None, incremental=True, return_params=False):
        """Raster-order sampling as base.AutoregressiveModel.sample (reference models/base.py:97-120: only the unknown
        entries replaced), with the draw made from the logistic mixture. Images live in [-1, 1]; entries of
        `conditioned_on` below -1 are the unknown ones. `image_size` (H, W) is needed when the model has not seen a
        batch yet.

        incremental=True (extension): the network is evaluated on the CURRENT ROW only (_row_net: the levels due at that
        row, against the convolutions' band caches) and a pixel is drawn by one kernel (ops.dmol_sample) from uniforms
        drawn up front by ONE torch.rand of shape (H * W, N, K + 3); the row step is captured into at most three step
        and three commit hipGraphs (rows with y % 4 == 0, y % 4 == 2, odd y) and replayed, eagerly launched when capture
        is refused. Pixels at which no image has an unknown entry are skipped; a row without any runs its commit pass only.
        incremental=False: one full forward per pixel and sample_from_mixture (the reference procedure).
        return_params=True (incremental only): every pixel is evaluated and the call returns (canvas, params), params
        the (N, 10 K, H, W) mixture parameters the draws were made from.
        A `sample_fn` given to the constructor replaces the mixture draw on the incremental path:
        sample_fn(params (N, 10 K)) -> (N, 3), called eagerly once per pixel."""
        self._no_input_codes()  # (the row-cached sampler runs _row_net, not _net)
        if return_params and not incremental:
            raise ValueError("return_params requires incremental=True")
        if conditioned_on is not None:
            canvas = conditioned_on.clone()
        else:
            assert n_samples is not None, 'Must provided one, and only one, of "n_samples" or "conditioned_on"'
            h, w = image_size if image_size is not None else (int(self._h), int(self._w))
            canvas = torch.full((n_samples, 3, h, w), -2.0, device=self.device)
        n, _, h, w = canvas.shape
        unknown = canvas < -1.0
        canvas = torch.where(unknown, torch.zeros_like(canvas), canvas)  # any finite value: later pixels are never read
        if incremental and (n >= self._incremental_min_batch or return_params):
            return self._sample_rows(canvas, unknown, return_params)
        for row in range(h):
            for col in range(w):
                if not bool(unknown[:, :, row, col].any()):
                    continue
                params = self._net(canvas)[:, :, row, col]
                drawn = self.sample_from_mixture(params, self._n_mix)
                canvas[:, :, row, col] = torch.where(unknown[:, :, row, col], drawn, canvas[:, :, row, col])
        return canvas

    def _sample_rows(self, canvas, unknown, return_params):
        n, _, h, w = canvas.shape
        if h % 4 or w % 4:
            raise ValueError("PixelCNNpp: H and W must be multiples of 4 (two stride-2 levels)")
        k, dev = self._n_mix, canvas.device
        fn = self._pixel_sample_fn
        canvas, unknown = canvas.contiguous(), unknown.contiguous()
        wanted = unknown.any(dim=0).any(dim=0).cpu()  # (H, W): the ONE host sync of the call
        wanted = [[True] * w for _ in range(h)] if return_params else wanted.tolist()
        uniforms = torch.rand((h * w, n, k + 3), device=dev) if fn is None else None
        params_map = torch.zeros((n, 10 * k, h, w), device=dev) if return_params else None
        row_in = torch.zeros((n, 3, 1, w), device=dev)
        pos_dev = torch.zeros(1, dtype=torch.int32, device=dev)  # the raster position the captured draw reads

        def step(ctx, target, host_pos=None):
            """The parameters of row ctx.row and (without a sample_fn) the draw of one pixel of `target` from them"""
            out = self._row_net(ctx, row_in)
            if fn is None and not ctx.commit:
                r, c = host_pos if host_pos is not None else (0, 0)
                ops.dmol_sample(out, uniforms, target, unknown, k, r, c, row_buf=row_in if target is canvas else None,
                                pos_dev=pos_dev if host_pos is None else None)
            return out

        ops.RowDecode.drop_caches(self)
        with ops.RowDecode(h) as ctx:
            # The row step differs only by which levels are due: three row classes (deepest level evaluated -> a row of that
            # class), each with a step graph (row forward + the draw at pos_dev) and a commit graph
            scratch = canvas.clone() if self._row_graph else None  # the warm-up's draws land here
            graphs = self._capture_row_steps(ctx, lambda: step(ctx, canvas), {2: 0, 1: 2, 0: 1},
                                             warm_step=lambda: step(ctx, scratch))
            schedule = row_schedule(h)
            for row in range(h):
                cls = schedule[row][-1][0]
                ctx.row, ctx.commit = row, False
                row_in.copy_(canvas[:, :, row:row + 1, :])
                for col in range(w):
                    if not wanted[row][col]:
                        continue
                    if graphs is not None:
                        pos_dev.fill_(row * w + col)
                        graphs[cls][0].replay()
                        out = graphs[cls][2]
                    else:
                        out = step(ctx, canvas, (row, col))
                    if return_params:
                        params_map[:, :, row, col] = out[:, :, 0, col]
                    if fn is not None:
                        drawn = fn(out[:, :, 0, col]).view(n, 3).to(canvas.dtype)
                        canvas[:, :, row, col] = torch.where(unknown[:, :, row, col], drawn, canvas[:, :, row, col])
                        row_in[:, :, 0, col] = canvas[:, :, row, col]
                ctx.commit = True  # the row is final: push it into every band (row_in already holds it)
                if graphs is not None:
                    graphs[cls][1].replay()
                else:
                    step(ctx, canvas)
        ops.RowDecode.drop_caches(self)
        return (canvas, params_map) if return_params else canvas


class PixelCNNppUnitRange(PixelCNNpp):
    """PixelCNNpp for loaders that deliver images in [0, 1] (the recipe's model): forward() maps its input to the
    network's [-1, 1]; sample() takes / returns images in [0, 1] (negative entries of `conditioned_on` are the
    unknown ones, as in the reference's base.AutoregressiveModel.sample, models/base.py:97-120) and runs the
    sampler's conditioning forwards on the UNSCALED network body."""

    def forward(self, x):
        return self._net(x * 2.0 - 1.0)

    @torch.no_grad()
    def sample(self, n_samples=None, conditioned_on=None, *, image_size=None, incremental=True, return_params=False):
        if conditioned_on is not None:
            conditioned_on = torch.where(conditioned_on < 0, torch.full_like(conditioned_on, -2.0),
                                         conditioned_on * 2.0 - 1.0)
        out = super().sample(n_samples, conditioned_on, image_size=image_size, incremental=incremental,
                             return_params=return_params)
        if return_params:
            return (out[0] + 1.0) * 0.5, out[1]
        return (out + 1.0) * 0.5


def dmol_loss(x, _, preds, n_mix=10):
    """loss_fn(x, y, preds) of the recipe: images in [0, 1] (the loaders' range) are mapped to [-1, 1]."""
    return ops.dmol_loss_sum_mean(preds, x * 2.0 - 1.0, n_mix)


def reproduce(n_epochs=457, batch_size=16, log_dir="/tmp/run", n_gpus=1, device_id=0, debug_loader=None,
              n_filters=160, n_resnet=5, n_mix=10):
    """Training recipe in the shape of the reference's reproduce() functions (there is no PixelCNN++ in the
    reference): CIFAR-10-shaped batches, the paper's model size by default, Adam lr 1e-3 with the per-batch
    decay 0.999995 of the paper, the discretized logistic mixture loss. Returns the Trainer."""
    from pytorch_generative_amd import recipes

    return recipes.run(
        lambda: PixelCNNppUnitRange(in_channels=3, n_filters=n_filters, n_resnet=n_resnet, n_mix=n_mix),
        loaders=lambda b: recipes.datasets.get_cifar10_loaders(b), loss_fn=lambda x, y, p: dmol_loss(x, y, p, n_mix),
        lr=1e-3, lr_decay=0.999995, n_epochs=n_epochs, batch_size=batch_size, log_dir=log_dir, n_gpus=n_gpus,
        device_id=device_id, debug_loader=debug_loader)
