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

``ModelTrainer`` below trains the encoder as well, with its BatchNorm statistics frozen (include/vfn_encoder_train.h holds that
definition and the formulas of one MBConv block's backward; ``freeze_encoder='statistics'`` in ``train_image_seg``):

    model.train(); model.encoder.eval()      # encoder: running statistics, no drop-connect; decoder BatchNorms: batch statistics
    for p in model.parameters(): p.requires_grad_(True)
    optimizer = torch.optim.Adam([dict(params=model.parameters(), lr=init_lr)])

    trainer = ModelTrainer(model, init_lr=1e-4)
    taps = trainer.encoder_forward(x)             # the stem's and the four stages' features, NHWC, channel-padded
    grads = trainer.encoder_backward(gfeats)      # 413 gradients by state-dict name from the gradients of the five taps

``FullTrainer`` at the end trains the encoder in train mode (include/vfn_encoder_bn_train.h holds that definition;
``freeze_encoder='train'``): batch-statistics BatchNorm in all 95 encoder BatchNorms, drop-connect in the residual blocks.

    model.train()
    trainer = FullTrainer(model, init_lr=1e-4, seed=0)
    logs = trainer.step(x, y)                     # keep=None: the drop-connect scales are drawn from trainer.generator

Not built: graph capture of the step, the BatchNorm apply fused into the next convolution's operand read.
"""
import torch

from . import _lib, ops, weights as W
from ._lib import ptr, stream, check
from .engine import choose_cfg, apply_choice, WS_FLOATS
from .linknet import BN_EPS_DEC, DEC_CHANNELS, STAGE_IDXS, LinknetB4, _blocks, _cp, _same_pad_before
from .train import AdamW
from .val_image_seg import seg_scores

BN_MOMENTUM = 0.1
# (freeze_encoder=False is the reference's spelling of 'train'; tests pin its refusal, so making it an alias is a follow-up that edits them)
ENCODER_MISSING = ("freeze_encoder=False is not accepted: the encoder in train mode (batch-statistics BatchNorm and drop-connect beside its "
                   "depthwise and squeeze-excite backward) is spelled freeze_encoder='train'; pass freeze_encoder='statistics' to train it with "
                   'frozen BatchNorm statistics, or freeze_encoder=True')
# in smp's state dict, not in its encoder's forward: no gradient, no optimizer state, they never move (as under torch's Adam)
UNUSED = ('encoder._conv_head.weight', 'encoder._bn1.weight', 'encoder._bn1.bias')


class Adam(AdamW):
    """``torch.optim.Adam([dict(params=..., lr=lr)])`` (train_image_seg.py:139-141; torch defaults: betas (0.9, 0.999), eps 1e-8,
    no weight decay) over the parameters that require a gradient: ``train.AdamW``'s flat buffer and kernel with
    ``weight_decay = 0``, the same arithmetic.  ``state_dict()`` has ``torch.optim.Adam``'s layout, parameters numbered in
    ``model.parameters()`` order, so the reference resumes from it and the other way round.  The learning rate is the attribute
    ``lr`` (the reference's ``optimizer.param_groups[0]['lr'] = 1e-5`` is ``optimizer.lr = 1e-5`` here)."""

    def __init__(self, named_params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, skip=()):
        """``skip``: names of parameters that require a gradient and never receive one: torch numbers them in the group and
        keeps no state for them; so does ``state_dict()`` here."""
        named = [(n, p) for n, p in named_params if p.requires_grad]
        super().__init__([(n, p) for n, p in named if n not in skip], lr=lr, betas=betas, eps=eps, weight_decay=0.0)
        everyone = [n for n, _ in named]
        self.n_group = len(everyone)                               # the size of torch's parameter group
        self.index = [everyone.index(n) for n in self.names]      # position in the group of each optimised parameter

    def state_dict(self):
        sd = super().state_dict()
        group = dict(torch.optim.Adam([torch.zeros(1)], lr=self.lr, betas=self.betas, eps=self.eps).state_dict()['param_groups'][0])
        group.update(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=0.0, params=list(range(self.n_group)))
        if self.initial_lr is not None:
            group['initial_lr'] = self.initial_lr
        sd['state'] = {self.index[i]: st for i, st in sd['state'].items()}
        sd['param_groups'] = [group]
        return sd

    def load_state_dict(self, sd):
        groups = sd['param_groups']
        if len(groups) != 1 or len(groups[0]['params']) != self.n_group:
            raise ValueError(f"loaded state dict has {sum(len(g['params']) for g in groups)} parameters in {len(groups)} group(s), "
                             f'this optimizer has {self.n_group} in one')
        ids = groups[0]['params']
        state = {i: sd['state'][ids[j]] for i, j in enumerate(self.index) if ids[j] in sd['state']}
        super().load_state_dict({'state': state, 'param_groups': [dict(groups[0], params=list(range(len(self.names))))]})


def freeze_encoder(model):
    """``model.train(); model.encoder.eval()`` and no gradient for the encoder's parameters."""
    model.train()
    model.encoder.eval()
    for p in model.encoder.parameters():
        p.requires_grad_(False)
    return model


def freeze_encoder_statistics(model):
    """``model.train(); model.encoder.eval()`` and a gradient for every parameter: the encoder trains on its running statistics,
    without drop-connect."""
    model.train()
    model.encoder.eval()
    for p in model.parameters():
        p.requires_grad_(True)
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
        self.model, self.dev = self._mode(model), dev
        self.optimizer = optimizer if optimizer is not None else self._new_optimizer(model, init_lr)
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

    _mode = staticmethod(freeze_encoder)

    @staticmethod
    def _new_optimizer(model, init_lr):
        return Adam(model.named_parameters(), lr=init_lr)

    def _encoder_taps(self, x):
        """The stem's and the four stages' features from the inference launch list."""
        taps = []
        self.model._predict_eager(self._encoder_pack(), x, True, taps=taps)
        return taps[:5]

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

    def _bn_backward(self, l, g, x, M, out=None):
        """g = dL/dy (overwritten with dL/dx of the raw convolution output, unless ``out`` takes it); dgamma, dbeta into the
        layer's buffers."""
        L = _lib.lib()
        C = l.cout_p
        check(L.vfn_lnt_bn_bwd_reduce_f32(ptr(g), ptr(x), ptr(l.scale), ptr(l.shift), ptr(l.mean), ptr(l.rstd), M, C, C, C, 1, ptr(self.part),
                                          ptr(l.dgamma), ptr(l.dbeta), stream()), 'vfn_lnt_bn_bwd_reduce_f32')
        check(L.vfn_lnt_bn_bwd_apply_f32(ptr(g), ptr(x), ptr(l.scale), ptr(l.shift), ptr(l.mean), ptr(l.rstd), ptr(l.dgamma), ptr(l.dbeta),
                                         ptr(g if out is None else out), M, C, C, C, C, 1, stream()), 'vfn_lnt_bn_bwd_apply_f32')
        return g if out is None else out

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
        feats = self._encoder_taps(x)[::-1]                    # deepest first: 448, 160, 56, 32, 48 channels
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
    def _backward(self, feat_grads=None):
        """dL/d(parameter) for the 52 trained tensors, by state-dict name (views of the kernels' packed outputs).  ``feat_grads``: a
        list that receives dL/d(feature) of the five encoder features, shallowest (the stem's) first: a skip add passes the
        gradient to both sides, so a skip feature's gradient is the block output's, kept from the in-place BatchNorm backward."""
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
            if feat_grads is not None and j + 1 < len(self.layers):
                feat_grads.append(g)
                g = self._bn_backward(lc, g, B['c_raw'], Mo, out=torch.empty_like(g))
            else:
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
            if j > 0 or feat_grads is not None:
                gx = torch.empty(N, h, w, la.cin_p, device=self.dev, dtype=torch.float32)
                self._conv(g, la.w_dgrad, la.cin_p, 1, 1, 0, gx, None, N, h, w)
                g = gx
        if feat_grads is not None:
            feat_grads.append(g)
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
    def forward_backward(self, x, y, feat_grads=None):
        """``pr = model(x); loss = DiceLoss()(pr, y); loss.backward()`` in training mode (the running statistics move, as they do
        in torch): ``(loss, grads)``, the loss a 0-dim f64 tensor on the device, the gradients by state-dict name.  ``feat_grads``:
        a list that receives dL/d(feature) of the five encoder features (``_backward``)."""
        with torch.cuda.device(self.dev):
            _, row = self._forward(x, y)
            grads = self._backward() if feat_grads is None else self._backward(feat_grads)
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


# ------------------------------------------------------------------------------------------------ the encoder trains as well
def _chunks(M, nmax):
    """The chunk count of a sum over M rows (include/vfn_encoder_train.h, "determinism")."""
    nb = min(nmax, -(-M // 64))
    rows = -(-M // nb)
    return -(-M // rows)


class _BN:
    """An eval-mode BatchNorm with trainable gamma / beta over ``cpad`` channels (zeros in the padding): gamma, beta,
    rstd = 1 / sqrt(running_var + eps), nshift = -running_mean rstd, fold = gamma rstd -- rows of the trainer's one table, filled
    for all layers at once by ``ModelTrainer._pack_bns`` -- and the two gradients."""

    def __init__(self, name, bn, cpad, dev):
        self.name, self.bn, self.c, self.cpad = name, bn, bn.weight.numel(), cpad
        self.gamma = self.beta = self.rstd = self.nshift = self.fold = None
        self.dgamma, self.dbeta = torch.zeros(cpad, device=dev), torch.zeros(cpad, device=dev)


class ModelTrainer(DecoderTrainer):
    """``ModelTrainer(model, init_lr)``: ``DecoderTrainer`` with the encoder trained as well on its running statistics
    (``freeze_encoder='statistics'``; the definition heads include/vfn_encoder_train.h).  ``Adam`` runs over the 465 tensors that
    receive a gradient; its ``state_dict()`` numbers all 468 of ``model.parameters()``.  The same public surface, and the two
    halves of the encoder's pass on their own: ``encoder_forward`` and ``encoder_backward``."""

    _mode = staticmethod(freeze_encoder_statistics)
    _fold_known = True          # gamma rstd is known before the forward pass (running statistics): the data-gradient filters are packed with it

    @staticmethod
    def _new_optimizer(model, init_lr):
        return Adam(model.named_parameters(), lr=init_lr, skip=UNUSED)

    def __init__(self, model, init_lr=1e-4, optimizer=None):
        super().__init__(model, init_lr=init_lr, optimizer=optimizer)
        dev, e = self.dev, model.encoder
        self.stem_bn = _BN('encoder._bn0', e._bn0, 64, dev)
        self.enc = []
        for i, (b, m) in enumerate(zip(_blocks(), e._blocks)):
            oup = b['cin'] * b['e']
            q = dict(b, i=i, m=m, name=f'encoder._blocks.{i}', oup=oup, cin_p=_cp(b['cin']), oup_p=_cp(oup), cout_p=_cp(b['cout']),
                     pad_b=_same_pad_before(b['k'], b['s']), residual=b['s'] == 1 and b['cin'] == b['cout'])
            if b['e'] != 1:
                q['bn0'] = _BN(q['name'] + '._bn0', m._bn0, q['oup_p'], dev)
            q['bn1'] = _BN(q['name'] + '._bn1', m._bn1, q['oup_p'], dev)
            q['bn2'] = _BN(q['name'] + '._bn2', m._bn2, q['cout_p'], dev)
            q['dw_w'] = torch.zeros(b['k'] ** 2, q['oup_p'], device=dev)
            self.enc.append(q)
        self.bns = [self.stem_bn] + [q[key] for q in self.enc for key in ('bn0', 'bn1', 'bn2') if key in q]
        self.bn_table = torch.zeros(5, sum(b.cpad for b in self.bns), device=dev)
        cols, off = [], 0
        for b in self.bns:
            b.gamma, b.beta, b.rstd, b.nshift, b.fold = (self.bn_table[r, off:off + b.cpad] for r in range(5))
            cols.append(torch.arange(off, off + b.c))
            off += b.cpad
        self.bn_cols = torch.cat(cols).to(dev)
        cmax = max(q['oup_p'] for q in self.enc)                                        # 2688: the widest layer sizes the scratch
        self.et_part = torch.empty(_lib.ET_MAX_BLOCKS * 2 * cmax, dtype=torch.float64, device=dev)
        self.wg_part = None
        self.esaved = None

    # -- what follows the parameters ------------------------------------------------------------------------------------
    def _pack_encoder(self):
        """Packed forward and data-gradient filters with the BatchNorm factors folded, rebuilt from the parameters (parameter-sized
        torch operations): the forward filter's epilogue is (rstd, -mean rstd), the data-gradient filter is
        (diag(gamma rstd) W)^T."""
        dev = self.dev
        self._pack_bns()
        self.stem_w = self.model.encoder._conv_stem.weight.detach().contiguous()
        for q in self.enc:
            m = q['m']
            for key, conv, bn, ci_p, co_p in (('exp', getattr(m, '_expand_conv', None), q.get('bn0'), q['cin_p'], q['oup_p']),
                                             ('proj', m._project_conv, q['bn2'], q['oup_p'], q['cout_p'])):
                if conv is None:
                    continue
                w = conv.weight.detach()
                if key + '_fwd' not in q:                       # (zero rows / columns in the padding, written once)
                    q[key + '_fwd'] = torch.zeros((co_p + 255) // 256 * 256, ci_p, device=dev)
                    q[key + '_dgrad'] = torch.zeros((ci_p + 255) // 256 * 256, co_p, device=dev)
                q[key + '_fwd'][:w.shape[0], :w.shape[1]] = w.view(w.shape[0], w.shape[1])
                if self._fold_known:
                    q[key + '_dgrad'][:ci_p] = (q[key + '_fwd'][:co_p] * bn.fold[:, None]).t()
            k2 = q['k'] ** 2
            q['dw_w'][:, :q['oup']] = m._depthwise_conv.weight.detach().view(q['oup'], k2).t()
            if self._fold_known:
                q['dw_fold'] = q['dw_w'] * q['bn1'].fold
            q['se'] = (m._se_reduce.weight.detach().view(q['sq'], q['oup']), m._se_reduce.bias.detach(),
                       m._se_expand.weight.detach().view(q['oup'], q['sq']), m._se_expand.bias.detach())

    def _pack_bns(self):
        """The table of every encoder BatchNorm's five vectors in a dozen operations (the encoder's eps is one number)."""
        cat = lambda f: torch.cat([f(b.bn).detach().float() for b in self.bns])
        gamma, beta, mean, var = cat(lambda m: m.weight), cat(lambda m: m.bias), cat(lambda m: m.running_mean), cat(lambda m: m.running_var)
        rstd = 1.0 / torch.sqrt(var + self.stem_bn.bn.eps)
        self.bn_table[:, self.bn_cols] = torch.stack([gamma, beta, rstd, -mean * rstd, gamma * rstd])

    # -- launches ---------------------------------------------------------------------------------------------------------
    def _conv1x1(self, x, wp, cout_p, out, scale, shift, N, h, w, res=None):
        LinknetB4._conv({'ws': self.ws}, x, wp, cout_p, 1, 0, out, scale, shift, N, h, w, res=res)

    def _affine(self, x, bn, y, M, C, res=None, swish=0):
        check(_lib.lib().vfn_et_affine_f32(ptr(x), ptr(bn.gamma), ptr(bn.beta), ptr(res), ptr(y), M, C, C, C, C, swish, stream()),
              'vfn_et_affine_f32')

    def _bn_grads(self, grads, bn, g, xh, M, C, keep=None, fresh=False):
        """dbeta = sum g, dgamma = sum g xhat; -> the gradient the weight and data gradients take under ``bn.fold``: g itself, the
        statistics are constants here (``keep``, ``fresh``: ``FullTrainer``'s)."""
        check(_lib.lib().vfn_et_colsums_f32(ptr(g), ptr(xh), 1, M, C, C, C, ptr(self.et_part), ptr(bn.dbeta), ptr(bn.dgamma), stream()),
              'vfn_et_colsums_f32')
        grads[bn.name + '.weight'], grads[bn.name + '.bias'] = bn.dgamma[:bn.c].clone(), bn.dbeta[:bn.c].clone()
        return g

    def _wgrad_1x1(self, x, g, cin_p, cout_p, rowscale, N, h, w):
        """[cout_p, cin_p] = diag(rowscale) g^T x over the pixels (a 1x1 convolution does not care how they are arranged; the
        weight gradient's pixel walk wants two per row: a single pixel gets a zero pixel beside it)."""
        M = N * h * w
        if M == 1:
            x, g = torch.cat([x.view(1, cin_p), x.new_zeros(1, cin_p)]), torch.cat([g.view(1, cout_p), g.new_zeros(1, cout_p)])
            M = 2
        if w >= 2 and M == N * h * w:
            return ops.conv_wgrad(x, g, 1, 1, 0, cin=cin_p, cout=cout_p, rowscale=rowscale, N=N, H=h, W=w)
        return ops.conv_wgrad(x.view(1, 1, M, cin_p), g.view(1, 1, M, cout_p), 1, 1, 0, cin=cin_p, cout=cout_p, rowscale=rowscale, N=1, H=1, W=M)

    # -- the encoder's two halves -------------------------------------------------------------------------------------------
    @torch.no_grad()
    def encoder_forward(self, x):
        """x f32 [N,3,H,W] -> the five taps (the stem's output and the four stages'; NHWC, channel-padded, as ``_predict_eager``'s
        ``taps``), from the parameters as they stand; keeps what ``encoder_backward`` needs."""
        _lib.require_gpu(x, 'x')
        if x.dim() != 4 or x.shape[1] != 3:
            raise RuntimeError(f'expected a normalised RGB batch [N,3,H,W], got {tuple(x.shape)}')
        if x.shape[2] % 32 or x.shape[3] % 32 or x.shape[2] < 32 or x.shape[3] < 32:
            raise RuntimeError(f'input height and width must be divisible by 32 (5 stride-2 stages), got {tuple(x.shape[2:])}')
        with torch.cuda.device(self.dev):
            return self._encoder_forward(x)

    def _encoder_forward(self, x):
        L = _lib.lib()
        self._pack_encoder()
        x = x.float().contiguous()
        N, H, Wd = x.shape[0], x.shape[2], x.shape[3]
        f = lambda *s: torch.empty(*s, device=self.dev, dtype=torch.float32)
        h, w = H // 2, Wd // 2
        sb = self.stem_bn
        xh = f(N, h, w, 64)
        check(L.vfn_et_stem_f32(ptr(x), ptr(self.stem_w), ptr(sb.rstd), ptr(sb.nshift), ptr(xh), N, H, Wd, h, w, 64, 64, _same_pad_before(3, 2),
                                stream()), 'vfn_et_stem_f32')
        cur = f(N, h, w, 64)
        self._affine(xh, sb, cur, N * h * w, 64, swish=1)
        saved, taps, need = [], [cur], 0
        for q in self.enc:
            inp, C = cur, q['oup_p']
            S = dict(x=inp, h=h, w=w)
            if q['e'] != 1:
                S['xh0'] = f(N, h, w, C)
                self._conv1x1(inp, q['exp_fwd'], C, S['xh0'], q['bn0'].rstd, q['bn0'].nshift, N, h, w)
                S['y0'] = f(N, h, w, C)
                self._affine(S['xh0'], q['bn0'], S['y0'], N * h * w, C)
            else:
                S['y0'] = inp
            ho, wo = h // q['s'], w // q['s']
            M = ho * wo
            b1 = q['bn1']
            S['xh1'] = f(N, ho, wo, C)
            check(L.vfn_et_dwconv_f32(ptr(S['y0']), ptr(q['dw_w']), ptr(b1.rstd), ptr(b1.nshift), ptr(S['xh1']), N, h, w, C, C, C, q['k'], q['s'],
                                      q['pad_b'], ho, wo, int(q['e'] != 1), stream()), 'vfn_et_dwconv_f32')
            S['a1'] = f(N, ho, wo, C)
            self._affine(S['xh1'], b1, S['a1'], N * M, C, swish=1)
            S['spx'], S['gate'] = f(N, C), f(N, C)
            check(L.vfn_et_colsums_f32(ptr(S['a1']), None, N, M, C, C, C, ptr(self.et_part), ptr(S['spx']), None, stream()), 'vfn_et_colsums_f32')
            w1, c1, w2, c2 = q['se']
            check(L.vfn_ln_se_gate_batch_f32(ptr(S['spx']), 1, 1.0 / M, ptr(w1), ptr(c1), ptr(w2), ptr(c2), ptr(S['gate']), N, q['oup'], q['sq'], C,
                                             stream()), 'vfn_ln_se_gate_batch_f32')
            S['s'] = f(N, ho, wo, C)
            check(L.vfn_et_scale_rows_f32(ptr(S['a1']), ptr(S['gate']), ptr(S['s']), N, M, C, C, C, stream()), 'vfn_et_scale_rows_f32')
            S['xh2'] = f(N, ho, wo, q['cout_p'])
            self._conv1x1(S['s'], q['proj_fwd'], q['cout_p'], S['xh2'], q['bn2'].rstd, q['bn2'].nshift, N, ho, wo)
            out = f(N, ho, wo, q['cout_p'])
            self._affine(S['xh2'], q['bn2'], out, N * M, q['cout_p'], res=inp if q['residual'] else None)
            need = max(need, _chunks(N * h * w, _lib.ET_MAX_BLOCKS) * q['k'] ** 2 * C)
            saved.append(S)
            cur, h, w = out, ho, wo
            if q['i'] + 1 in STAGE_IDXS:
                taps.append(cur)
        if self.wg_part is None or self.wg_part.numel() < need:
            self.wg_part = torch.empty(need, dtype=torch.float64, device=self.dev)
        self.esaved = dict(blocks=saved, x=x, xh_stem=xh, N=N, H=H, W=Wd)
        return taps

    @torch.no_grad()
    def encoder_backward(self, gfeats):
        """gfeats: dL/d(tap) of the five taps of the last ``encoder_forward``, in their layout (not written to) -> the 413 gradients
        of ``encoder.*`` by state-dict name.  A stage feature's gradient joins where the walk passes that stage's last block; a
        residual block passes the gradient to its input and to its branch."""
        if self.esaved is None:
            raise RuntimeError('encoder_backward follows encoder_forward')
        if len(gfeats) != 5:
            raise ValueError(f'expected the gradients of the five taps, got {len(gfeats)}')
        with torch.cuda.device(self.dev):
            grads = self._encoder_backward([g.contiguous() for g in gfeats])
        self.esaved = None
        return grads

    def _encoder_backward(self, gfeats):
        L = _lib.lib()
        E = self.esaved
        N = E['N']
        f = lambda *s: torch.empty(*s, device=self.dev, dtype=torch.float32)
        grads, stage, g = {}, 4, None
        for q, S in zip(self.enc[::-1], E['blocks'][::-1]):
            h, w, C, cout_p, k = S['h'], S['w'], q['oup_p'], q['cout_p'], q['k']
            ho, wo = h // q['s'], w // q['s']
            M, Mo, Mi = ho * wo, N * ho * wo, N * h * w
            if q['i'] + 1 in STAGE_IDXS:                            # this block's output is a tap
                t = gfeats[stage]
                if t.shape != (N, ho, wo, cout_p) or t.dtype != torch.float32 or not t.is_cuda:
                    raise ValueError(f'gradient of tap {stage}: expected f32 {(N, ho, wo, cout_p)} on the GPU, got {t.dtype} {tuple(t.shape)}')
                if g is None:
                    g = t
                else:
                    check(L.vfn_ln_add_f32(ptr(g), ptr(t), ptr(g), g.numel(), stream()), 'vfn_ln_add_f32')
                stage -= 1
            name, b1, b2 = q['name'], q['bn1'], q['bn2']
            # the project convolution behind its BatchNorm
            gb = self._bn_grads(grads, b2, g, S['xh2'], Mo, cout_p, keep=S.get('keep'), fresh=True)
            dw = self._wgrad_1x1(S['s'], gb, C, cout_p, b2.fold, N, ho, wo)
            grads[name + '._project_conv.weight'] = dw[:q['cout'], :q['oup']].unsqueeze(-1).unsqueeze(-1)
            gs = f(N, ho, wo, C)
            self._conv1x1(gb, q['proj_dgrad'], C, gs, None, None, N, ho, wo)
            # squeeze-excite
            dgate, dpool, tmp = f(N, C), f(N, C), f(N * (C + 2 * q['sq']))
            check(L.vfn_et_colsums_f32(ptr(gs), ptr(S['a1']), N, M, C, C, C, ptr(self.et_part), None, ptr(dgate), stream()), 'vfn_et_colsums_f32')
            w1, c1, w2, c2 = q['se']
            dw1, db1, dw2, db2 = f(q['sq'], q['oup'], 1, 1), f(q['sq']), f(q['oup'], q['sq'], 1, 1), f(q['oup'])
            check(L.vfn_et_se_bwd_f32(ptr(S['spx']), 1.0 / M, ptr(dgate), ptr(w1), ptr(c1), ptr(w2), ptr(c2), ptr(tmp), ptr(dpool), ptr(dw1), ptr(db1),
                                      ptr(dw2), ptr(db2), N, q['oup'], q['sq'], C, stream()), 'vfn_et_se_bwd_f32')
            grads[name + '._se_reduce.weight'], grads[name + '._se_reduce.bias'] = dw1, db1
            grads[name + '._se_expand.weight'], grads[name + '._se_expand.bias'] = dw2, db2
            # the gate, the pooling and the swish behind the depthwise BatchNorm: one pass, in place
            check(L.vfn_et_swish_bwd_f32(ptr(gs), ptr(S['gate']), ptr(dpool), 1.0 / M, ptr(S['xh1']), ptr(b1.gamma), ptr(b1.beta), ptr(gs), N, M, C, C,
                                         C, C, stream()), 'vfn_et_swish_bwd_f32')
            gs = self._bn_grads(grads, b1, gs, S['xh1'], Mo, C)
            # the depthwise convolution
            act = int(q['e'] != 1)
            dwd = f(k * k, C)
            check(L.vfn_et_dw_wgrad_f32(ptr(gs), ptr(S['y0']), ptr(self.wg_part), ptr(dwd), N, h, w, C, C, C, k, q['s'], q['pad_b'], ho, wo, act,
                                        stream()), 'vfn_et_dw_wgrad_f32')
            grads[name + '._depthwise_conv.weight'] = (dwd * b1.fold)[:, :q['oup']].t().reshape(q['oup'], 1, k, k)
            gy0 = f(N, h, w, C)
            check(L.vfn_et_dw_dgrad_f32(ptr(gs), ptr(q['dw_fold']), ptr(S['y0']) if act else None, ptr(gy0), N, h, w, C, C, C, C, k, q['s'], q['pad_b'],
                                        ho, wo, act, stream()), 'vfn_et_dw_dgrad_f32')
            if act:
                b0 = q['bn0']
                gy0 = self._bn_grads(grads, b0, gy0, S['xh0'], Mi, C)
                dw = self._wgrad_1x1(S['x'], gy0, q['cin_p'], C, b0.fold, N, h, w)
                grads[name + '._expand_conv.weight'] = dw[:q['oup'], :q['cin']].unsqueeze(-1).unsqueeze(-1)
                gx = f(N, h, w, q['cin_p'])
                self._conv1x1(gy0, q['exp_dgrad'], q['cin_p'], gx, None, None, N, h, w, res=g if q['residual'] else None)
            else:
                gx = gy0
                if q['residual']:
                    check(L.vfn_ln_add_f32(ptr(gx), ptr(g), ptr(gx), gx.numel(), stream()), 'vfn_ln_add_f32')
            g = gx
        # the stem: its tap's gradient, the swish, the BatchNorm, the weight gradient (no data gradient)
        t, sb = gfeats[0], self.stem_bn
        h, w = E['H'] // 2, E['W'] // 2
        if t.shape != (N, h, w, 64) or t.dtype != torch.float32 or not t.is_cuda:
            raise ValueError(f'gradient of tap 0: expected f32 {(N, h, w, 64)} on the GPU, got {t.dtype} {tuple(t.shape)}')
        check(L.vfn_ln_add_f32(ptr(g), ptr(t), ptr(g), g.numel(), stream()), 'vfn_ln_add_f32')
        check(L.vfn_et_swish_bwd_f32(ptr(g), None, None, 1.0, ptr(E['xh_stem']), ptr(sb.gamma), ptr(sb.beta), ptr(g), 1, N * h * w, 64, 64, 64, 64,
                                     stream()), 'vfn_et_swish_bwd_f32')
        g = self._bn_grads(grads, sb, g, E['xh_stem'], N * h * w, 64)
        dws = f(48, 27)
        check(L.vfn_et_stem_wgrad_f32(ptr(g), ptr(E['x']), ptr(self.et_part), ptr(dws), N, E['H'], E['W'], h, w, 64, _same_pad_before(3, 2), stream()),
              'vfn_et_stem_wgrad_f32')
        grads['encoder._conv_stem.weight'] = (dws * sb.fold[:48, None]).view(48, 3, 3, 3)
        return grads

    # -- the decoder's pass between them --------------------------------------------------------------------------------------
    def _encoder_taps(self, x):
        return self._encoder_forward(x)

    def _backward(self, feat_grads=None):
        fg = []
        grads = super()._backward(feat_grads=fg)
        grads.update(self._encoder_backward(fg))
        self.esaved = None
        if feat_grads is not None:
            feat_grads.extend(fg)
        return grads


# ------------------------------------------------------------------------------------------------ the encoder in train mode
DROP_CONNECT_RATE = 0.2          # efficientnet_pytorch: block i of n has rate DROP_CONNECT_RATE * i / n


def train_mode(model):
    """``model.train()`` and a gradient for every parameter: every BatchNorm on batch statistics, drop-connect on."""
    model.train()
    for p in model.parameters():
        p.requires_grad_(True)
    return model


def drop_connect_rates():
    """(block index, rate) of the blocks that run under drop-connect: residual (stride 1, cin == cout) and rate > 0."""
    blocks = _blocks()
    return [(i, DROP_CONNECT_RATE * i / len(blocks)) for i, b in enumerate(blocks) if b['s'] == 1 and b['cin'] == b['cout'] and i > 0]


def keep_table(u):
    """u [blocks under drop-connect][N] uniform in [0, 1) -> the scale of each image's branch: floor(1 - p + u) / (1 - p), that is
    0 or 1 / (1 - p).  float32."""
    p = torch.tensor([r for _, r in drop_connect_rates()], dtype=torch.float64)[:, None]
    if u.dim() != 2 or u.shape[0] != p.shape[0]:
        raise ValueError(f'expected one row of draws per block under drop-connect ({p.shape[0]}), got {tuple(u.shape)}')
    return (torch.floor(1.0 - p + u.double()) / (1.0 - p)).float()


class FullTrainer(ModelTrainer):
    """``FullTrainer(model, init_lr, seed=0)``: ``ModelTrainer`` with the encoder in train mode (``freeze_encoder='train'``; the
    definition heads include/vfn_encoder_bn_train.h): its 95 BatchNorms normalise with the batch's statistics and move their
    running ones on the device, the residual blocks run under drop-connect.  Each convolution leaves its raw output,
    ``vfn_et_bn_stats_f32`` writes rstd, -mean rstd and gamma rstd into the BatchNorm table and ``vfn_et_bn_norm_f32`` normalises
    (xhat in place of the raw output) and applies gamma, beta, the activation, the drop-connect scale and the residual; the
    backward centres each BatchNorm's gradient (``vfn_et_bn_center_f32``) between the column sums and the weight and data
    gradients, whose folded filters are formed at the head of the backward, when gamma rstd is known.

    ``keep``: the drop-connect scales [blocks under drop-connect][N] (``keep_table``); None draws them from ``generator``, a host
    ``torch.Generator`` (``reseed``).  They travel to the device in one pinned asynchronous copy at the head of the step."""

    _mode = staticmethod(train_mode)
    _fold_known = False

    def __init__(self, model, init_lr=1e-4, optimizer=None, seed=0):
        super().__init__(model, init_lr=init_lr, optimizer=optimizer)
        for b in self.bns:
            m = b.bn
            if m.momentum is None or not m.track_running_stats or m.running_mean.dtype != torch.float32 or not m.running_mean.is_contiguous():
                raise ValueError(f'{b.name}: a BatchNorm with a momentum and contiguous float32 running statistics is expected')
        self.drop = dict(drop_connect_rates())                     # block index -> rate
        self.drop_row = {i: r for r, i in enumerate(self.drop)}
        cmax = self.et_part.numel() // (_lib.ET_MAX_BLOCKS * 2)
        self.ones, self.zeros = torch.ones(cmax, device=self.dev), torch.zeros(cmax, device=self.dev)
        self.generator = torch.Generator()
        self.seed = seed
        self.reseed(0)
        self._keep_arg, self._keep_host, self._keep_copied = None, None, torch.cuda.Event()

    def reseed(self, epoch):
        """The drop-connect draws of an epoch follow from (seed, epoch): a resumed run continues the sequence."""
        self.generator.manual_seed((int(self.seed) * 1000003 + int(epoch)) % (1 << 63))

    # -- what follows the parameters ------------------------------------------------------------------------------------
    def _pack_bns(self):
        """gamma and beta only: rstd, -mean rstd and gamma rstd are written by the statistics kernel."""
        cat = lambda f: torch.cat([f(b.bn).detach().float() for b in self.bns])
        self.bn_table[:2, self.bn_cols] = torch.stack([cat(lambda m: m.weight), cat(lambda m: m.bias)])

    def _fold(self):
        """The data-gradient filters (diag(gamma rstd) W)^T and the folded depthwise filter, from the batch's rstd."""
        for q in self.enc:
            for key, bn, ci_p, co_p in (('exp', q.get('bn0'), q['cin_p'], q['oup_p']), ('proj', q['bn2'], q['oup_p'], q['cout_p'])):
                if bn is not None:
                    q[key + '_dgrad'][:ci_p] = (q[key + '_fwd'][:co_p] * bn.fold[:, None]).t()
            q['dw_fold'] = q['dw_w'] * q['bn1'].fold

    def _take_keep(self, N):
        """The step's table on the device, [blocks under drop-connect][N]."""
        keep, self._keep_arg = self._keep_arg, None
        R = len(self.drop)
        if keep is None:
            keep = keep_table(torch.rand(R, N, generator=self.generator, dtype=torch.float64))
        if tuple(keep.shape) != (R, N):
            raise ValueError(f'keep: expected the scales of {R} blocks and {N} images, got {tuple(keep.shape)}')
        if keep.is_cuda:
            return keep.to(self.dev, torch.float32).contiguous()
        if self._keep_host is None or self._keep_host.shape != (R, N):
            self._keep_host = torch.empty(R, N, dtype=torch.float32, pin_memory=True)
        self._keep_copied.synchronize()                          # (the last step's copy: long done)
        self._keep_host.copy_(keep)
        dev = torch.empty(R, N, dtype=torch.float32, device=self.dev)
        dev.copy_(self._keep_host, non_blocking=True)
        self._keep_copied.record()
        return dev

    # -- launches ---------------------------------------------------------------------------------------------------------
    def _bn_train(self, bn, z, y, B, M, C, swish=0, keep=None, res=None):
        """z: the raw convolution output, xhat when this returns; y = act(gamma xhat + beta) keep (+ res)."""
        L = _lib.lib()
        m = bn.bn
        check(L.vfn_et_bn_stats_f32(ptr(z), B * M, C, C, ptr(bn.gamma), m.eps, m.momentum, ptr(self.et_part), ptr(bn.rstd), ptr(bn.nshift),
                                    ptr(bn.fold), ptr(m.running_mean), ptr(m.running_var), bn.c, stream()), 'vfn_et_bn_stats_f32')
        check(L.vfn_et_bn_norm_f32(ptr(z), ptr(bn.rstd), ptr(bn.nshift), ptr(bn.gamma), ptr(bn.beta), ptr(keep), ptr(res), ptr(z), ptr(y), B, M, C,
                                   C, C, C, C, swish, stream()), 'vfn_et_bn_norm_f32')

    def _bn_grads(self, grads, bn, g, xh, M, C, keep=None, fresh=False):
        """dbeta = sum keep g, dgamma = sum keep g xhat; -> g' = keep g - dbeta / M - xhat dgamma / M: in place, or a new tensor
        (``fresh``: g is a caller's tensor, or a residual block's pass-through)."""
        L = _lib.lib()
        N = self.esaved['N']
        if keep is None:
            check(L.vfn_et_colsums_f32(ptr(g), ptr(xh), 1, M, C, C, C, ptr(self.et_part), ptr(bn.dbeta), ptr(bn.dgamma), stream()), 'vfn_et_colsums_f32')
        else:
            sg, sga = torch.empty(N, C, device=self.dev), torch.empty(N, C, device=self.dev)
            check(L.vfn_et_colsums_f32(ptr(g), ptr(xh), N, M // N, C, C, C, ptr(self.et_part), ptr(sg), ptr(sga), stream()), 'vfn_et_colsums_f32')
            check(L.vfn_et_bn_sums_f32(ptr(sg), ptr(sga), ptr(keep), ptr(bn.dbeta), ptr(bn.dgamma), N, C, stream()), 'vfn_et_bn_sums_f32')
        grads[bn.name + '.weight'], grads[bn.name + '.bias'] = bn.dgamma[:bn.c].clone(), bn.dbeta[:bn.c].clone()
        gp = torch.empty_like(g) if fresh or keep is not None else g
        check(L.vfn_et_bn_center_f32(ptr(g), ptr(xh), ptr(keep), ptr(bn.dbeta), ptr(bn.dgamma), ptr(gp), N, M // N, C, C, C, C, stream()),
              'vfn_et_bn_center_f32')
        return gp

    # -- the encoder's two halves -------------------------------------------------------------------------------------------
    def encoder_forward(self, x, keep=None):
        """``ModelTrainer.encoder_forward`` in train mode: the running statistics move and the counters count."""
        self._keep_arg = keep
        try:
            taps = super().encoder_forward(x)
        finally:
            self._keep_arg = None
        self._invalidate()
        return taps

    def _encoder_forward(self, x):
        L = _lib.lib()
        N, H, Wd = x.shape[0], x.shape[2], x.shape[3]
        if N * (H // 32) * (Wd // 32) < 2:         # the deepest BatchNorms see one value per channel: torch's own refusal
            raise ValueError(f'Expected more than 1 value per channel when training, got input size {[N, 448, H // 32, Wd // 32]}')
        keep = self._take_keep(N)
        self._pack_encoder()
        x = x.float().contiguous()
        f = lambda *s: torch.empty(*s, device=self.dev, dtype=torch.float32)
        h, w = H // 2, Wd // 2
        sb = self.stem_bn
        xh = f(N, h, w, 64)
        check(L.vfn_et_stem_f32(ptr(x), ptr(self.stem_w), ptr(self.ones), ptr(self.zeros), ptr(xh), N, H, Wd, h, w, 64, 64, _same_pad_before(3, 2),
                                stream()), 'vfn_et_stem_f32')
        cur = f(N, h, w, 64)
        self._bn_train(sb, xh, cur, N, h * w, 64, swish=1)
        saved, taps, need = [], [cur], 0
        for q in self.enc:
            inp, C = cur, q['oup_p']
            S = dict(x=inp, h=h, w=w)
            if q['e'] != 1:
                S['xh0'] = f(N, h, w, C)
                self._conv1x1(inp, q['exp_fwd'], C, S['xh0'], None, None, N, h, w)
                S['y0'] = f(N, h, w, C)
                self._bn_train(q['bn0'], S['xh0'], S['y0'], N, h * w, C)
            else:
                S['y0'] = inp
            ho, wo = h // q['s'], w // q['s']
            M = ho * wo
            S['xh1'] = f(N, ho, wo, C)
            check(L.vfn_et_dwconv_f32(ptr(S['y0']), ptr(q['dw_w']), ptr(self.ones), ptr(self.zeros), ptr(S['xh1']), N, h, w, C, C, C, q['k'], q['s'],
                                      q['pad_b'], ho, wo, int(q['e'] != 1), stream()), 'vfn_et_dwconv_f32')
            S['a1'] = f(N, ho, wo, C)
            self._bn_train(q['bn1'], S['xh1'], S['a1'], N, M, C, swish=1)
            S['spx'], S['gate'] = f(N, C), f(N, C)
            check(L.vfn_et_colsums_f32(ptr(S['a1']), None, N, M, C, C, C, ptr(self.et_part), ptr(S['spx']), None, stream()), 'vfn_et_colsums_f32')
            w1, c1, w2, c2 = q['se']
            check(L.vfn_ln_se_gate_batch_f32(ptr(S['spx']), 1, 1.0 / M, ptr(w1), ptr(c1), ptr(w2), ptr(c2), ptr(S['gate']), N, q['oup'], q['sq'], C,
                                             stream()), 'vfn_ln_se_gate_batch_f32')
            S['s'] = f(N, ho, wo, C)
            check(L.vfn_et_scale_rows_f32(ptr(S['a1']), ptr(S['gate']), ptr(S['s']), N, M, C, C, C, stream()), 'vfn_et_scale_rows_f32')
            S['xh2'] = f(N, ho, wo, q['cout_p'])
            self._conv1x1(S['s'], q['proj_fwd'], q['cout_p'], S['xh2'], None, None, N, ho, wo)
            out = f(N, ho, wo, q['cout_p'])
            if q['i'] in self.drop:
                S['keep'] = keep[self.drop_row[q['i']]]
            self._bn_train(q['bn2'], S['xh2'], out, N, M, q['cout_p'], keep=S.get('keep'), res=inp if q['residual'] else None)
            need = max(need, _chunks(N * h * w, _lib.ET_MAX_BLOCKS) * q['k'] ** 2 * C)
            saved.append(S)
            cur, h, w = out, ho, wo
            if q['i'] + 1 in STAGE_IDXS:
                taps.append(cur)
        torch._foreach_add_([b.bn.num_batches_tracked for b in self.bns], 1)
        if self.wg_part is None or self.wg_part.numel() < need:
            self.wg_part = torch.empty(need, dtype=torch.float64, device=self.dev)
        self.esaved = dict(blocks=saved, x=x, xh_stem=xh, N=N, H=H, W=Wd, keep=keep)
        return taps

    def _encoder_backward(self, gfeats):
        self._fold()
        return super()._encoder_backward(gfeats)

    # -- the public steps ----------------------------------------------------------------------------------------------------
    def forward_backward(self, x, y, feat_grads=None, keep=None):
        self._keep_arg = keep
        try:
            return super().forward_backward(x, y, feat_grads)
        finally:
            self._keep_arg = None

    def step(self, x, y, keep=None):
        """``ModelTrainer.step`` with the step's drop-connect scales (None: drawn from ``generator``)."""
        self._keep_arg = keep
        try:
            return super().step(x, y)
        finally:
            self._keep_arg = None
