"""Fine-tuning the bootstrap LinkNet's decoder and head on the HIP path, with the encoder frozen (include/vfn_image_train.h
holds the definition).  In torch terms:

    model.train(); model.encoder.eval()
    for p in model.encoder.parameters(): p.requires_grad_(False)
    optimizer = torch.optim.Adam([dict(params=[p for p in model.parameters() if p.requires_grad], lr=init_lr)])
    # per batch:  pr = model(x); loss = DiceLoss()(pr, y); optimizer.zero_grad(); loss.backward(); optimizer.step()

    trainer = DecoderTrainer(model, init_lr=1e-4)
    logs = trainer.step(x, y)          # {'dice_loss', 'iou_score'}: 0-dim f64 tensors that stay on the device until asked for

One step:

* the encoder's features come from ``LinknetB4._predict_eager`` (the inference launch list: folded running statistics, no
  drop-connect) through its ``taps``; the encoder receives no gradient;
* the 15 decoder convolutions run through ``vfn_conv2d_nhwc_f32`` with unit scale (the transposed convolution's bias in the
  shift), each followed by batch-statistics BatchNorm: ``vfn_lnt_bn_stats_f32`` (mean, biased variance, scale, shift, the
  running statistics' momentum update) and ``vfn_lnt_bn_apply_f32`` (+ ReLU); the head is ``vfn_ln_head_f32``;
* ``vfn_seg_scores_f64`` leaves S0 .. S4, the Dice loss and the IoU on the device; ``vfn_lnt_head_bwd_f32`` reads the sums there;
* backwards per layer: ``vfn_lnt_bn_bwd_reduce_f32`` (dgamma, dbeta), ``vfn_lnt_bn_bwd_apply_f32`` (the gradient of the raw
  convolution output), ``vfn_conv_wgrad_f32`` (weights; the transposed convolution as the 4x4 convolution of the zero-inserted
  input, mapped back to ``Wt[i][o][kh][kw]``), ``vfn_colsum_f32`` (the transposed convolution's bias) and the data gradient
  through ``vfn_conv2d_nhwc_f32``: the transposed filter matrix for a 1x1 layer, and for the transposed convolution the
  4x4 / stride-2 / pad-1 convolution of the gradient with ``Wd[i][(kh, kw, o)] = Wt[i][o][kh][kw]`` -- the implicit-GEMM tile
  configurations take any stride, so that route is the one taken (no gather of a stride-1 result).  Block 0's first
  convolution needs no data gradient; the skip adds pass the gradient through;
* ``Adam`` below is ``train.AdamW`` with ``weight_decay = 0`` (one ``vfn_adamw_f32`` launch over the 52 tensors in one flat
  buffer) whose ``state_dict()`` has ``torch.optim.Adam``'s layout.

The packed forward and data-gradient filters and the padded BatchNorm parameters are rebuilt from the parameters at the head
of every forward pass (torch operations on parameter-sized tensors only), so they follow ``optimizer.step()`` and a
``load_state_dict`` alike; no torch operation touches an activation-sized tensor inside a step.  The head's bias travels to
``vfn_ln_head_f32`` as a host float: it is copied to pinned memory at the head of the step and waited for just before the
head's launch, when the whole forward pass is already enqueued.  There is no CPU fallback.

Not built: gradients for the encoder (batch-statistics BatchNorm, drop-connect, depthwise and squeeze-excite backward there),
graph capture of the step, the BatchNorm apply fused into the next convolution's operand read.
"""
import torch

from . import _lib, ops, weights as W
from ._lib import ptr, stream, check
from .engine import choose_cfg, apply_choice, WS_FLOATS
from .linknet import BN_EPS_DEC, DEC_CHANNELS, LinknetB4, _cp
from .train import AdamW
from .val_image_seg import seg_scores

BN_MOMENTUM = 0.1
ENCODER_MISSING = ('training the encoder is not built: batch-statistics BatchNorm, drop-connect, depthwise and squeeze-excite '
                   'backward in the encoder are missing; pass freeze_encoder=True')


class Adam(AdamW):
    """``torch.optim.Adam([dict(params=..., lr=lr)])`` (train_image_seg.py:139-141; torch defaults: betas (0.9, 0.999), eps 1e-8,
    no weight decay) over the parameters that require a gradient: ``train.AdamW``'s flat buffer and kernel with
    ``weight_decay = 0``, the same arithmetic.  ``state_dict()`` has ``torch.optim.Adam``'s layout, parameters numbered in
    ``model.parameters()`` order, so the reference resumes from it and the other way round.  The learning rate is the attribute
    ``lr`` (the reference's ``optimizer.param_groups[0]['lr'] = 1e-5`` is ``optimizer.lr = 1e-5`` here)."""

    def __init__(self, named_params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8):
        super().__init__(named_params, lr=lr, betas=betas, eps=eps, weight_decay=0.0)

    def state_dict(self):
        sd = super().state_dict()
        group = dict(torch.optim.Adam([torch.zeros(1)], lr=self.lr, betas=self.betas, eps=self.eps).state_dict()['param_groups'][0])
        group.update(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=0.0, params=list(range(len(self.names))))
        if self.initial_lr is not None:
            group['initial_lr'] = self.initial_lr
        sd['param_groups'] = [group]
        return sd


def freeze_encoder(model):
    """``model.train(); model.encoder.eval()`` and no gradient for the encoder's parameters."""
    model.train()
    model.encoder.eval()
    for p in model.encoder.parameters():
        p.requires_grad_(False)
    return model


class _Layer:
    """One convolution + BatchNorm of a decoder block: the modules, the padded sizes and the device buffers of its statistics."""

    def __init__(self, name, conv, bn, kind, cin_p, cout_p, dev):
        self.name, self.conv, self.bn, self.kind, self.cin_p, self.cout_p = name, conv, bn, kind, cin_p, cout_p
        self.c = bn.weight.numel()
        z = lambda: torch.zeros(cout_p, device=dev)
        self.gamma, self.beta, self.bias = z(), z(), (z() if kind == 't' else None)
        self.scale, self.shift, self.mean, self.rstd, self.dgamma, self.dbeta = z(), z(), z(), z(), z(), z()
        self.run_mean, self.run_var = z(), z()
        self.w_fwd = self.w_dgrad = None


class DecoderTrainer:
    """``DecoderTrainer(model, init_lr)``: ``model`` a ``LinknetB4`` on the GPU.  The constructor freezes the encoder (above) and
    builds ``Adam`` over the 52 tensors of ``decoder.*`` and ``segmentation_head.0.*`` (``optimizer``: one built before, e.g.
    restored from a checkpoint).  After a step ``model.predict`` / ``predict_batch`` and ``model.state_dict()`` use the new
    parameters and running statistics."""

    def __init__(self, model, init_lr=1e-4, optimizer=None):
        if not isinstance(model, LinknetB4):
            raise TypeError('DecoderTrainer trains a linknet.LinknetB4')
        dev = next(model.parameters()).device
        if dev.type != 'cuda':
            raise RuntimeError('DecoderTrainer runs on hand-written HIP kernels only: move the model to the GPU (no CPU fallback)')
        _lib.lib()
        self.model, self.dev = freeze_encoder(model), dev
        self.optimizer = optimizer if optimizer is not None else Adam(model.named_parameters(), lr=init_lr)
        self.layers = []
        for j, blk in enumerate(model.decoder.blocks):
            cin, cout = DEC_CHANNELS[j], DEC_CHANNELS[j + 1]
            cin_p, mid_p, cout_p = _cp(cin), _cp(cin // 4), _cp(cout)
            p = f'decoder.blocks.{j}.block'
            self.layers.append([_Layer(f'{p}.0', blk.block[0][0], blk.block[0][1], 'a', cin_p, mid_p, dev),
                                _Layer(f'{p}.1', blk.block[1][0], blk.block[1][1], 't', mid_p, mid_p, dev),
                                _Layer(f'{p}.2', blk.block[2][0], blk.block[2][1], 'c', mid_p, cout_p, dev)])
        self.head_w = torch.zeros(32, device=dev)
        self.head_gw, self.head_gb = torch.zeros(32, device=dev), torch.zeros(1, device=dev)
        self._head_b = torch.empty(1, dtype=torch.float32, pin_memory=True)
        self._head_b_ready = torch.cuda.Event()
        self.ws = torch.empty(WS_FLOATS, device=dev)
        self.part = torch.empty(_lib.LNT_MAX_BLOCKS * 2 * 256, dtype=torch.float64, device=dev)      # (decoder layers: <= 160 channels)
        self.colsum_part = torch.empty(256 * 256, device=dev)
        self.scores_part = torch.empty(_lib.SEG_SCORES_MAX_BLOCKS * 5, dtype=torch.float64, device=dev)
        self._enc, self._enc_token, self._enc_tensors = None, None, None
        self.saved = None

    # -- what follows the parameters ------------------------------------------------------------------------------------
    def _encoder_pack(self):
        """The model's packed weights with an empty decoder list: ``_predict_eager`` then runs the encoder's launches alone (and
        its head over the deepest feature, one launch whose result nobody reads).  Packed once: the encoder is frozen; a
        ``load_state_dict`` or a move of the model (the tensors' versions / addresses change) packs again."""
        e = self.model.encoder
        if self._enc_tensors is None:
            self._enc_tensors = list(e.parameters()) + list(e.buffers())
        token = (sum(t._version for t in self._enc_tensors), e._conv_stem.weight.data_ptr())
        if self._enc is None or self._enc_token != token:
            self._enc = dict(self.model._pack(), dec=[])
            self.model._packed = None
            self._enc_token = token
        return self._enc

    def _seat_running_stats(self):
        """The modules' running statistics live in the first C floats of the padded buffers the statistics kernel updates."""
        for blk in self.layers:
            for l in blk:
                for name, buf in (('running_mean', l.run_mean), ('running_var', l.run_var)):
                    cur = getattr(l.bn, name)
                    if cur.data_ptr() != buf.data_ptr() or cur.device != buf.device:
                        buf[:l.c].copy_(cur)
                        setattr(l.bn, name, buf[:l.c])

    def _pack(self):
        """Everything the launches read that is derived from the parameters (parameter-sized torch operations)."""
        dev = self.dev
        for blk in self.layers:
            for l in blk:
                l.gamma[:l.c].copy_(l.bn.weight.detach())
                l.beta[:l.c].copy_(l.bn.bias.detach())
                w = l.conv.weight.detach().float()
                if l.kind == 't':                                   # Wt [in, out, 4, 4]
                    mid = w.shape[0]
                    l.bias[:mid].copy_(l.conv.bias.detach())
                    wc = torch.zeros(l.cout_p, l.cin_p, 4, 4, device=dev)
                    wc[:mid, :mid] = w.flip(2, 3).transpose(0, 1)   # linknet.pack_transposed: Wc[o][i][kh][kw] = Wt[i][o][3-kh][3-kw]
                    wd = torch.zeros(l.cin_p, l.cout_p, 4, 4, device=dev)
                    wd[:mid, :mid] = w                              # data gradient: filter i over the gradient's channels o
                    l.w_fwd, l.w_dgrad = ops.pad_rows(W.pack_conv_weight(wc)), ops.pad_rows(W.pack_conv_weight(wd))
                else:
                    cout, cin = w.shape[0], w.shape[1]
                    full = torch.zeros(l.cout_p, l.cin_p, device=dev)
                    full[:cout, :cin] = w.view(cout, cin)
                    l.w_fwd, l.w_dgrad = ops.pad_rows(full), ops.pad_rows(full.t().contiguous())
        head = self.model.segmentation_head[0]
        self.head_w.copy_(head.weight.detach().view(32))
        self._head_b.copy_(head.bias.detach(), non_blocking=True)
        self._head_b_ready.record()

    # -- launches ---------------------------------------------------------------------------------------------------------
    def _conv(self, x, wp, cout_p, k, stride, pad, out, shift, N, H, Wd, Ho=None, Wo=None, table=True):
        d = ops.make_conv_desc(x, wp, cout_p, k, k, stride, pad, out, None, shift, None, False, False, N=N, H=H, W=Wd)
        if Ho is not None:
            d.Ho, d.Wo, d.M = Ho, Wo, N * Ho * Wo
        choice = choose_cfg(d.M, d.Cout, d.KH * d.KW * d.Cin, 0, use_table=table)
        if choice[1] > 1 and d.out_ld % 4:
            choice = (choice[0], 1, 0)
        ops.conv2d_launch(d, apply_choice(d, choice, self.ws, None), 0)

    def _bn_forward(self, l, x, M, track):
        L = _lib.lib()
        check(L.vfn_lnt_bn_stats_f32(ptr(x), M, l.cout_p, l.cout_p, ptr(l.gamma), ptr(l.beta), BN_EPS_DEC, BN_MOMENTUM, ptr(self.part),
                                     ptr(l.scale), ptr(l.shift), ptr(l.mean), ptr(l.rstd), ptr(l.run_mean) if track else None,
                                     ptr(l.run_var) if track else None, stream()), 'vfn_lnt_bn_stats_f32')
        y = torch.empty_like(x)
        check(L.vfn_lnt_bn_apply_f32(ptr(x), ptr(l.scale), ptr(l.shift), ptr(y), M, l.cout_p, l.cout_p, l.cout_p, 1, stream()),
              'vfn_lnt_bn_apply_f32')
        if track:
            l.bn.num_batches_tracked += 1
        return y

    def _bn_backward(self, l, g, x, M):
        """g = dL/dy (overwritten with dL/dx of the raw convolution output); dgamma, dbeta into the layer's buffers."""
        L = _lib.lib()
        C = l.cout_p
        check(L.vfn_lnt_bn_bwd_reduce_f32(ptr(g), ptr(x), ptr(l.scale), ptr(l.shift), ptr(l.mean), ptr(l.rstd), M, C, C, C, 1, ptr(self.part),
                                          ptr(l.dgamma), ptr(l.dbeta), stream()), 'vfn_lnt_bn_bwd_reduce_f32')
        check(L.vfn_lnt_bn_bwd_apply_f32(ptr(g), ptr(x), ptr(l.scale), ptr(l.shift), ptr(l.mean), ptr(l.rstd), ptr(l.dgamma), ptr(l.dbeta),
                                         ptr(g), M, C, C, C, C, 1, stream()), 'vfn_lnt_bn_bwd_apply_f32')
        return g

    def _check_inputs(self, x, y):
        _lib.require_gpu(x, 'x')
        _lib.require_gpu(y, 'y')
        if x.dim() != 4 or x.shape[1] != 3:
            raise RuntimeError(f'expected a normalised RGB batch [N,3,H,W], got {tuple(x.shape)}')
        N, H, Wd = x.shape[0], x.shape[2], x.shape[3]
        if H % 32 or Wd % 32 or H < 32 or Wd < 32:
            raise RuntimeError(f'input height and width must be divisible by 32 (5 stride-2 stages), got {tuple(x.shape[2:])}')
        if y.dtype != torch.float32 or y.numel() != N * H * Wd:
            raise ValueError(f'labels must be float32 [N,1,H,W] for x {tuple(x.shape)}, got {y.dtype} {tuple(y.shape)}')
        if N * (H // 32) * (Wd // 32) < 2:         # the deepest BatchNorm sees one value per channel: torch's own refusal
            raise ValueError(f'Expected more than 1 value per channel when training, got input size {[N, 112, H // 32, Wd // 32]}')

    @torch.no_grad()
    def _forward(self, x, y, track=True):
        """The training-mode forward pass; keeps what the backward needs in ``self.saved``.  Returns (sums f64 [5], [dice_loss,
        iou_score] f64 [2]) on the device."""
        self._check_inputs(x, y)
        L = _lib.lib()
        m = self.model
        self._seat_running_stats()
        self._pack()
        taps = []
        m._predict_eager(self._encoder_pack(), x, True, taps=taps)
        feats = taps[:5][::-1]                                 # deepest first: 448, 160, 56, 32, 48 channels
        N, h, w = x.shape[0], x.shape[2] // 32, x.shape[3] // 32
        f = lambda *s: torch.empty(*s, device=self.dev, dtype=torch.float32)
        xd, saved = feats[0], []
        for j, (la, lt, lc) in enumerate(self.layers):
            a_raw = f(N, h, w, la.cout_p)
            self._conv(xd, la.w_fwd, la.cout_p, 1, 1, 0, a_raw, None, N, h, w)
            a = self._bn_forward(la, a_raw, N * h * w, track)
            z = f(N, 2 * h, 2 * w, lt.cin_p)
            check(L.vfn_dilate2_f32(ptr(a), ptr(z), N, h, w, 2 * h, 2 * w, lt.cin_p, stream()), 'vfn_dilate2_f32')
            t_raw = f(N, 2 * h, 2 * w, lt.cout_p)
            self._conv(z, lt.w_fwd, lt.cout_p, 4, 1, 2, t_raw, lt.bias, N, 2 * h, 2 * w, Ho=2 * h, Wo=2 * w)
            t = self._bn_forward(lt, t_raw, N * 4 * h * w, track)
            c_raw = f(N, 2 * h, 2 * w, lc.cout_p)
            self._conv(t, lc.w_fwd, lc.cout_p, 1, 1, 0, c_raw, None, N, 2 * h, 2 * w)
            c = self._bn_forward(lc, c_raw, N * 4 * h * w, track)
            if j + 1 < len(feats):
                check(L.vfn_ln_add_f32(ptr(c), ptr(feats[j + 1]), ptr(c), c.numel(), stream()), 'vfn_ln_add_f32')
            saved.append(dict(x=xd, a_raw=a_raw, z=z, t_raw=t_raw, t=t, c_raw=c_raw, h=h, w=w))
            xd, h, w = c, 2 * h, 2 * w
        pr = f(N, 1, h, w)
        self._head_b_ready.synchronize()                        # (the bias' copy of _pack: long done, the forward pass is enqueued)
        check(L.vfn_ln_head_f32(ptr(xd), ptr(self.head_w), float(self._head_b[0]), ptr(pr), N * h * w, 32, xd.shape[-1], 1, stream()),
              'vfn_ln_head_f32')
        gt = y.contiguous()
        sums, row = seg_scores(pr, gt, 0.5, part=self.scores_part)
        self.saved = dict(blocks=saved, xd=xd, pr=pr, gt=gt, sums=sums, N=N)
        return sums, row

    @torch.no_grad()
    def _backward(self):
        """dL/d(parameter) for the 52 trained tensors, by state-dict name (views of the kernels' packed outputs)."""
        L = _lib.lib()
        S = self.saved
        N, xd = S['N'], S['xd']
        M = xd.shape[0] * xd.shape[1] * xd.shape[2]
        g = torch.empty(xd.shape[0], xd.shape[1], xd.shape[2], 32, device=self.dev, dtype=torch.float32)
        check(L.vfn_lnt_head_bwd_f32(ptr(xd), ptr(self.head_w), ptr(S['pr']), ptr(S['gt']), ptr(S['sums']), M, xd.shape[-1], ptr(self.part),
                                     ptr(g), ptr(self.head_gw), ptr(self.head_gb), stream()), 'vfn_lnt_head_bwd_f32')
        grads = {'segmentation_head.0.weight': self.head_gw.view(1, 32, 1, 1), 'segmentation_head.0.bias': self.head_gb}
        for j in range(len(self.layers) - 1, -1, -1):
            la, lt, lc = self.layers[j]
            B = S['blocks'][j]
            h, w = B['h'], B['w']
            Mo = N * 4 * h * w
            # the block's last 1x1 convolution (the skip add in front of g passes it through)
            g = self._bn_backward(lc, g, B['c_raw'], Mo)
            self._grads_1x1(grads, lc, B['t'], g, N, 2 * h, 2 * w)
            gt_ = torch.empty(N, 2 * h, 2 * w, lt.cout_p, device=self.dev, dtype=torch.float32)
            self._conv(g, lc.w_dgrad, lt.cout_p, 1, 1, 0, gt_, None, N, 2 * h, 2 * w)
            # the transposed convolution
            g = self._bn_backward(lt, gt_, B['t_raw'], Mo)
            mid = lt.c
            dw = ops.conv_wgrad(B['z'], g, 4, 1, 2, cin=lt.cin_p, cout=lt.cout_p, N=N, H=2 * h, W=2 * w)      # [o][(kh, kw, i)] of Wc
            grads[lt.name + '.0.weight'] = dw.view(lt.cout_p, 4, 4, lt.cin_p)[:mid, :, :, :mid].flip(1, 2).permute(3, 0, 1, 2)
            db = torch.empty(lt.cout_p, device=self.dev, dtype=torch.float32)
            check(L.vfn_colsum_f32(ptr(g), Mo, lt.cout_p, lt.cout_p, ptr(self.colsum_part), 256, ptr(db), stream()), 'vfn_colsum_f32')
            grads[lt.name + '.0.bias'] = db[:mid]
            grads[lt.name + '.1.weight'], grads[lt.name + '.1.bias'] = lt.dgamma[:mid].clone(), lt.dbeta[:mid].clone()
            ga = torch.empty(N, h, w, la.cout_p, device=self.dev, dtype=torch.float32)
            self._conv(g, lt.w_dgrad, la.cout_p, 4, 2, 1, ga, None, N, 2 * h, 2 * w, table=False)
            # the block's first 1x1 convolution
            g = self._bn_backward(la, ga, B['a_raw'], N * h * w)
            self._grads_1x1(grads, la, B['x'], g, N, h, w)
            if j > 0:
                gx = torch.empty(N, h, w, la.cin_p, device=self.dev, dtype=torch.float32)
                self._conv(g, la.w_dgrad, la.cin_p, 1, 1, 0, gx, None, N, h, w)
                g = gx
        self.saved = None
        return grads

    def _grads_1x1(self, grads, l, x, g, N, h, w):
        if w >= 2:
            dw = ops.conv_wgrad(x, g, 1, 1, 0, cin=l.cin_p, cout=l.cout_p, N=N, H=h, W=w)
        else:       # the weight gradient's pixel walk wants two pixels per row; a 1x1 convolution does not care how they are arranged
            M = N * h * w
            dw = ops.conv_wgrad(x.view(1, 1, M, l.cin_p), g.view(1, 1, M, l.cout_p), 1, 1, 0, cin=l.cin_p, cout=l.cout_p, N=1, H=1, W=M)
        c, cin = l.c, l.conv.weight.shape[1]
        grads[l.name + '.0.weight'] = dw[:c, :cin].unsqueeze(-1).unsqueeze(-1)
        grads[l.name + '.1.weight'], grads[l.name + '.1.bias'] = l.dgamma[:c].clone(), l.dbeta[:c].clone()

    # -- the public steps ----------------------------------------------------------------------------------------------------
    def forward_backward(self, x, y):
        """``pr = model(x); loss = DiceLoss()(pr, y); loss.backward()`` in training mode (the running statistics move, as they do
        in torch): ``(loss, grads)``, the loss a 0-dim f64 tensor on the device, the gradients by state-dict name."""
        with torch.cuda.device(self.dev):
            _, row = self._forward(x, y)
            grads = self._backward()
        self._invalidate()
        return row[0], grads

    def step(self, x, y):
        """One optimisation step on a batch: x f32 [N,3,H,W] (ImageNet-normalised), y f32 [N,1,H,W] in {0, 1}.  Returns smp's two
        logs of the training-mode prediction, on the device."""
        with torch.cuda.device(self.dev):
            _, row = self._forward(x, y)
            grads = self._backward()
            self.optimizer.set_grads(grads)
            self.optimizer.step()
        self._invalidate()
        return {'dice_loss': row[0], 'iou_score': row[1]}

    def _invalidate(self):
        """As ``LinknetB4.load_state_dict``: the inference path packs again and captures its graphs again."""
        self.model._packed = None
        self.model._graphs, self.model._graph_runs = {}, {}
