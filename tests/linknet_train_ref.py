"""Restatements, in plain torch on the CPU, of what ``csrc/image_train.hip`` and ``vfloodnet_amd/linknet_train.py`` compute
(include/vfn_image_train.h): the five kernel formulas in any dtype -- float64 is the reference, float32 the yardstick of the
error rule -- one decoder block's backward pass chained from them the way the product chains it, and the decoder under
``torch.autograd`` as the reference of the whole step.  ``tests/test_image_train_ref_host.py`` holds every function here
against ``torch.autograd``."""
import copy

import torch
import torch.nn.functional as F

BN_EPS, BN_MOMENTUM = 1e-5, 0.1


# ------------------------------------------------------------------------------------------------ the five kernel formulas
def bn_stats(x, gamma, beta, running_mean, running_var, eps=BN_EPS, momentum=BN_MOMENTUM):
    """x [M, C] -> dict(mean, var (biased), rstd, scale, shift, running_mean, running_var): two passes, in x's dtype."""
    M = x.shape[0]
    mean = x.sum(0) / M
    var = ((x - mean) ** 2).sum(0) / M
    rstd = 1 / torch.sqrt(var + eps)
    scale = gamma * rstd
    return dict(mean=mean, var=var, rstd=rstd, scale=scale, shift=beta - mean * scale,
                running_mean=(1 - momentum) * running_mean + momentum * mean,
                running_var=(1 - momentum) * running_var + momentum * var * M / (M - 1))


def bn_apply(x, scale, shift, relu=True):
    y = x * scale + shift
    return F.relu(y) if relu else y


def _masked(g, x, scale, shift, relu):
    return g * (x * scale + shift > 0).to(g.dtype) if relu else g


def bn_bwd_reduce(g, x, scale, shift, mean, rstd, relu=True):
    """-> (dgamma, dbeta, the summands' absolute sums): g' = g [y > 0], xhat = (x - mean) rstd."""
    gp = _masked(g, x, scale, shift, relu)
    xh = (x - mean) * rstd
    return (gp * xh).sum(0), gp.sum(0), (gp * xh).abs().sum(0), gp.abs().sum(0)


def bn_bwd_apply(g, x, scale, shift, mean, rstd, dgamma, dbeta, relu=True):
    M = x.shape[0]
    gp = _masked(g, x, scale, shift, relu)
    return scale * (gp - dbeta / M - (x - mean) * rstd * (dgamma / M))


def dice_sums(pr, gt):
    return (gt * pr).sum(), pr.sum(), gt.sum()


def dice_loss(pr, gt):
    s0, s1, s2 = dice_sums(pr, gt)
    return 1 - (2 * s0 + 1) / (s1 + s2 + 1)


def head_bwd(x, w, pr, gt, sums=None):
    """x [M, 32], w [32], pr, gt [M] -> (g_x [M, 32], g_w [32], g_b, sum |dz|): the head convolution, the sigmoid and the Dice
    loss backwards, from the probabilities of the forward pass."""
    s0, s1, s2 = dice_sums(pr, gt) if sums is None else sums
    D = s1 + s2 + 1
    dz = -(2 * gt * D - (2 * s0 + 1)) / (D * D) * pr * (1 - pr)
    return dz[:, None] * w[None, :], (dz[:, None] * x).sum(0), dz.sum(), dz.abs().sum()


# ------------------------------------------------------------------------ one decoder block, chained as the product chains it
def _rows(t):
    """[N, C, h, w] -> [M, C]."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _image(rows, N, h, w):
    return rows.reshape(N, h, w, -1).permute(0, 3, 1, 2)


def dilate2(a):
    """The zero-inserted input of the transposed convolution: out[.., 2y, 2x] = a[.., y, x]."""
    N, C, h, w = a.shape
    z = a.new_zeros(N, C, 2 * h, 2 * w)
    z[:, :, ::2, ::2] = a
    return z


def transposed_as_conv(a, wt, bias):
    """ConvTranspose2d(4, 2, 1): the stride-1 4x4 convolution of the zero-inserted input (2 zeros before, 1 after) with
    Wc[o][i][kh][kw] = Wt[i][o][3-kh][3-kw]."""
    wc = wt.flip(2, 3).transpose(0, 1)
    return F.conv2d(F.pad(dilate2(a), (2, 1, 2, 1)), wc, bias)


def block_forward_backward(x, params, g_out):
    """One decoder block in training mode and its backward pass from the formulas above and the convolution identities the product
    uses.  x [N, cin, h, w]; params: dict(w_a, g_a, b_a, wt, bias, g_t, b_t, w_c, g_c, b_c); g_out = dL/d(block output).  ->
    (output, dict of gradients by the same keys, dL/dx)."""
    N, _, h, w = x.shape
    dt = x.dtype
    zero = lambda c: torch.zeros(c, dtype=dt)
    # forward
    a_raw = F.conv2d(x, params['w_a'])
    sa = bn_stats(_rows(a_raw), params['g_a'], params['b_a'], zero(a_raw.shape[1]), zero(a_raw.shape[1]))
    a = _image(bn_apply(_rows(a_raw), sa['scale'], sa['shift']), N, h, w)
    t_raw = transposed_as_conv(a, params['wt'], params['bias'])
    st = bn_stats(_rows(t_raw), params['g_t'], params['b_t'], zero(t_raw.shape[1]), zero(t_raw.shape[1]))
    t = _image(bn_apply(_rows(t_raw), st['scale'], st['shift']), N, 2 * h, 2 * w)
    c_raw = F.conv2d(t, params['w_c'])
    sc = bn_stats(_rows(c_raw), params['g_c'], params['b_c'], zero(c_raw.shape[1]), zero(c_raw.shape[1]))
    out = _image(bn_apply(_rows(c_raw), sc['scale'], sc['shift']), N, 2 * h, 2 * w)
    grads = {}

    def bn_back(g, raw, s, kg, kb):
        dg, db, _, _ = bn_bwd_reduce(g, _rows(raw), s['scale'], s['shift'], s['mean'], s['rstd'])
        grads[kg], grads[kb] = dg, db
        return bn_bwd_apply(g, _rows(raw), s['scale'], s['shift'], s['mean'], s['rstd'], dg, db)

    # the last 1x1 convolution: weight gradient = g^T t over the pixels, data gradient = g W
    g = bn_back(_rows(g_out), c_raw, sc, 'g_c', 'b_c')
    grads['w_c'] = (g.t() @ _rows(t))[:, :, None, None]
    g = g @ params['w_c'][:, :, 0, 0]
    # the transposed convolution: weight gradient of the 4x4 convolution over the zero-inserted input, mapped back
    g = bn_back(g, t_raw, st, 'g_t', 'b_t')
    grads['bias'] = g.sum(0)
    gi = _image(g, N, 2 * h, 2 * w)
    zp = F.pad(dilate2(a), (2, 1, 2, 1))
    mid = a.shape[1]
    dwc = torch.zeros(mid, mid, 4, 4, dtype=dt)                    # dWc[o][i][kh][kw] = sum g[o][y][x] zp[i][y + kh][x + kw]
    for kh in range(4):
        for kw in range(4):
            dwc[:, :, kh, kw] = torch.einsum('noyx,niyx->oi', gi, zp[:, :, kh:kh + 2 * h, kw:kw + 2 * w])
    grads['wt'] = dwc.flip(2, 3).transpose(0, 1)                   # dWt[i][o][kh][kw] = dWc[o][i][3-kh][3-kw]
    # data gradient: the 4x4 / stride-2 / pad-1 convolution of g with filter i over the gradient's channels o: Wd[i][o] = Wt[i][o]
    ga = F.conv2d(gi, params['wt'], stride=2, padding=1)
    # the first 1x1 convolution
    g = bn_back(_rows(ga), a_raw, sa, 'g_a', 'b_a')
    grads['w_a'] = (g.t() @ _rows(x))[:, :, None, None]
    gx = _image(g @ params['w_a'][:, :, 0, 0], N, h, w)
    return out, grads, gx


# -------------------------------------------------------------------------------------------- the whole step under autograd
TRAINED_PREFIXES = ('decoder.', 'segmentation_head.0.')


def decoder_reference(model, feats, y, dtype=torch.float64):
    """``copy.deepcopy(model.decoder)`` and the head in ``dtype``, train mode, under autograd, fed with given features.
    feats: the encoder's five features deepest first [N, C, h, w] (448, 160, 56, 32, 48 channels); y [N, 1, H, W].  ->
    (loss, gradients by state-dict name, running statistics by state-dict name, probabilities, and for each transposed
    convolution's bias -- a gradient that is zero up to rounding, BatchNorm follows -- the sum of its summands' magnitudes)."""
    dec = copy.deepcopy(model.decoder).to('cpu').to(dtype).train()
    head = copy.deepcopy(model.segmentation_head).to('cpu').to(dtype)
    for p in list(dec.parameters()) + list(head.parameters()):
        p.requires_grad_(True)
        p.grad = None
    feats = [f.detach().to('cpu').to(dtype) for f in feats]
    abs_sums = {}
    def watch(name):
        def hook(module, inputs, output):
            output.register_hook(lambda g: abs_sums.__setitem__(name, g.detach().abs().sum((0, 2, 3))))
        return hook

    for j, blk in enumerate(dec.blocks):
        blk.block[1][0].register_forward_hook(watch(f'decoder.blocks.{j}.block.1.0.bias'))
    x = feats[0]
    for j, blk in enumerate(dec.blocks):
        x = blk.block(x)
        if j + 1 < len(feats):
            x = x + feats[j + 1]
    pr = torch.sigmoid(head(x))
    loss = dice_loss(pr, y.detach().to('cpu').to(dtype))
    loss.backward()
    grads = {'decoder.' + n: p.grad.detach() for n, p in dec.named_parameters()}
    grads.update({'segmentation_head.' + n: p.grad.detach() for n, p in head.named_parameters()})
    stats = {'decoder.' + n: b.detach().clone() for n, b in dec.named_buffers()}
    return loss.detach(), grads, stats, pr.detach(), abs_sums


def adam_step(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam's update in float64 -> (p, m, v)."""
    p, g, m, v = (t.double() for t in (p, g, m, v))
    m = betas[0] * m + (1 - betas[0]) * g
    v = betas[1] * v + (1 - betas[1]) * g * g
    denom = (v / (1 - betas[1] ** step)).sqrt() + eps
    return p - lr / (1 - betas[0] ** step) * m / denom, m, v
