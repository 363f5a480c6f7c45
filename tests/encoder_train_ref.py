"""Restatements, in plain torch on the CPU, of what ``csrc/encoder_train.hip`` and ``linknet_train.ModelTrainer`` compute
(include/vfn_encoder_train.h): each kernel's formula in any dtype -- float64 is the reference, float32 the yardstick of the
error rule -- and one MBConv block's backward pass chained from them the way the product chains it (both block forms: without
an expand convolution, and with a residual).  ``tests/test_encoder_train_ref_host.py`` holds every function here against
``torch.autograd``.  Activations are NHWC: [N, H, W, C], or [B, M, C] where only rows matter."""
import copy

import torch
import torch.nn.functional as F

BN_EPS_ENC = 1e-3
TAP_CHANNELS = (48, 32, 56, 160, 448)                          # the stem and the four stages
UNUSED = ('encoder._conv_head.weight', 'encoder._bn1.weight', 'encoder._bn1.bias')


def swish(x):
    return x * torch.sigmoid(x)


def dswish(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


# --------------------------------------------------------------------------------------------------- the kernel formulas
def affine(x, scale, shift, res=None, act=False):
    y = x * scale + shift
    if act:
        y = swish(y)
    return y if res is None else y + res


def scale_rows(x, gate):
    """x [B, M, C], gate [B, C]."""
    return x * gate[:, None, :]


def colsums(g, a=None):
    """g, a [B, M, C] -> (sum_m g, sum_m g a, and the summands' absolute sums), each [B, C]."""
    ga = g if a is None else g * a
    return g.sum(1), ga.sum(1), g.abs().sum(1), ga.abs().sum(1)


def se_gate(sum_px, inv_hw, w1, b1, w2, b2):
    """sum_px [B, C] -> (pooled mean, u, swish(u), gate)."""
    p = sum_px * inv_hw
    u = p @ w1.t() + b1
    hid = swish(u)
    return p, u, hid, torch.sigmoid(hid @ w2.t() + b2)


def se_bwd(sum_px, inv_hw, dgate, w1, b1, w2, b2):
    """-> dict(dpool [B, C] (gradient of the pooled mean), dw1 [sq, C], db1 [sq], dw2 [C, sq], db2 [C])."""
    p, u, hid, gate = se_gate(sum_px, inv_hw, w1, b1, w2, b2)
    dv = dgate * gate * (1 - gate)
    du = (dv @ w2) * dswish(u)
    return dict(dpool=du @ w1, dw1=du.t() @ p, db1=du.sum(0), dw2=dv.t() @ hid, db2=dv.sum(0))


def swish_bwd(g, xh, scale, shift, gate=None, dpool=None, inv_hw=1.0):
    """g, xh [B, M, C]; gate, dpool [B, C]."""
    if gate is not None:
        g = g * gate[:, None, :] + (dpool * inv_hw)[:, None, :]
    return g * dswish(xh * scale + shift)


def _embed(x, pad_b, Lh, Lw):
    """x [N, H, W, C] inside zeros [N, Lh, Lw, C] at offset pad_b (rows / columns that fall outside are cut off)."""
    N, H, W, C = x.shape
    out = x.new_zeros(N, Lh, Lw, C)
    h, w = min(H, Lh - pad_b), min(W, Lw - pad_b)
    out[:, pad_b:pad_b + h, pad_b:pad_b + w] = x[:, :h, :w]
    return out


def _window(P, ky, kx, s, Ho, Wo):
    return P[:, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s]


def dw_forward(x, w, k, s, pad_b, Ho, Wo):
    """The raw depthwise convolution of vfn_ln_dwconv_f32: x [N, H, W, C], w [k*k, C] tap-major -> [N, Ho, Wo, C]."""
    P = _embed(x, pad_b, (Ho - 1) * s + k, (Wo - 1) * s + k)
    return sum(_window(P, t // k, t % k, s, Ho, Wo) * w[t] for t in range(k * k))


def dw_dgrad(g, w, H, W, k, s, pad_b, y=None):
    """g [N, Ho, Wo, C] -> gx [N, H, W, C]; times swish'(y) when y (the tensor the forward kernel read) is given."""
    N, Ho, Wo, C = g.shape
    Lh, Lw = (Ho - 1) * s + k, (Wo - 1) * s + k
    GP = g.new_zeros(N, max(Lh, pad_b + H), max(Lw, pad_b + W), C)
    for t in range(k * k):
        _window(GP, t // k, t % k, s, Ho, Wo).add_(g * w[t])
    gx = GP[:, pad_b:pad_b + H, pad_b:pad_b + W]
    return gx if y is None else gx * dswish(y)


def dw_wgrad(g, a, k, s, pad_b, act=False):
    """-> (dw [k*k, C], the summands' absolute sums)."""
    N, Ho, Wo, C = g.shape
    P = _embed(swish(a) if act else a, pad_b, (Ho - 1) * s + k, (Wo - 1) * s + k)
    prods = [g * _window(P, t // k, t % k, s, Ho, Wo) for t in range(k * k)]
    return torch.stack([p.sum((0, 1, 2)) for p in prods]), torch.stack([p.abs().sum((0, 1, 2)) for p in prods])


def stem_patches(x, Ho, Wo, pad_b):
    """x [N, 3, H, W] -> [N, Ho, Wo, 27], taps ordered (ci, ky, kx) as the filter [48][3][3][3]."""
    P = _embed(x.permute(0, 2, 3, 1), pad_b, (Ho - 1) * 2 + 3, (Wo - 1) * 2 + 3)
    taps = [_window(P, ky, kx, 2, Ho, Wo) for ky in range(3) for kx in range(3)]      # each [N, Ho, Wo, 3]
    return torch.stack(taps, -1).reshape(x.shape[0], Ho, Wo, 27)                        # (ci, (ky, kx))


def stem_forward(x, w, scale, shift, Ho, Wo, pad_b):
    """-> [N, Ho, Wo, 48] = conv scale + shift, no activation."""
    return stem_patches(x, Ho, Wo, pad_b) @ w.reshape(48, 27).t() * scale + shift


def stem_wgrad(g, x, pad_b):
    """g [N, Ho, Wo, 48] -> (dw [48, 3, 3, 3], the summands' absolute sums)."""
    N, Ho, Wo, _ = g.shape
    v = stem_patches(x, Ho, Wo, pad_b).reshape(-1, 27)
    gr = g.reshape(-1, 48)
    return (gr.t() @ v).reshape(48, 3, 3, 3), (gr.abs().t() @ v.abs()).reshape(48, 3, 3, 3)


# ----------------------------------------------------------------------------- one MBConv block, chained as the product chains it
def bn_consts(p, prefix, eps=BN_EPS_ENC):
    rstd = 1 / torch.sqrt(p[prefix + '.running_var'] + eps)
    return rstd, -p[prefix + '.running_mean'] * rstd


def mbconv_params(cin, cout, k, e, sq, gen, dtype=torch.float64):
    """Random parameters of one block under efficientnet-pytorch's names (no prefix)."""
    oup = cin * e
    r = lambda *s: torch.randn(*s, generator=gen).to(dtype)
    p = {}
    def bn(name, c):
        p[name + '.weight'], p[name + '.bias'] = 1 + 0.2 * r(c), 0.2 * r(c)
        p[name + '.running_mean'], p[name + '.running_var'] = 0.3 * r(c), 0.5 + torch.rand(c, generator=gen).to(dtype)
    if e != 1:
        p['_expand_conv.weight'] = r(oup, cin, 1, 1) / cin ** 0.5
        bn('_bn0', oup)
    p['_depthwise_conv.weight'] = r(oup, 1, k, k) / k
    bn('_bn1', oup)
    p['_se_reduce.weight'], p['_se_reduce.bias'] = r(sq, oup, 1, 1) / oup ** 0.5, 0.2 * r(sq)
    p['_se_expand.weight'], p['_se_expand.bias'] = r(oup, sq, 1, 1) / sq ** 0.5, 0.2 * r(oup)
    p['_project_conv.weight'] = r(cout, oup, 1, 1) / oup ** 0.5
    bn('_bn2', cout)
    return p


def mbconv_forward(x, p, k, s, pad_b, e, residual, keep=None):
    """x [N, H, W, cin] -> the block's output [N, Ho, Wo, cout] from the formulas above (differentiable); ``keep``: a dict that
    receives what the product saves for the backward."""
    N, H, W, _ = x.shape
    Ho, Wo = H // s, W // s
    if e != 1:
        r0, h0 = bn_consts(p, '_bn0')
        xh0 = affine(x @ p['_expand_conv.weight'][:, :, 0, 0].t(), r0, h0)
        y0 = affine(xh0, p['_bn0.weight'], p['_bn0.bias'])
    else:
        xh0, y0 = None, x
    r1, h1 = bn_consts(p, '_bn1')
    oup = y0.shape[-1]
    wdw = p['_depthwise_conv.weight'].reshape(oup, k * k).t()
    xh1 = affine(dw_forward(swish(y0) if e != 1 else y0, wdw, k, s, pad_b, Ho, Wo), r1, h1)
    a1 = affine(xh1, p['_bn1.weight'], p['_bn1.bias'], act=True).reshape(N, Ho * Wo, oup)
    sq = p['_se_reduce.bias'].numel()
    sum_px = colsums(a1)[0]
    se = (p['_se_reduce.weight'].reshape(sq, oup), p['_se_reduce.bias'], p['_se_expand.weight'].reshape(oup, sq), p['_se_expand.bias'])
    gate = se_gate(sum_px, 1.0 / (Ho * Wo), *se)[3]
    sg = scale_rows(a1, gate)
    r2, h2 = bn_consts(p, '_bn2')
    xh2 = affine(sg @ p['_project_conv.weight'][:, :, 0, 0].t(), r2, h2).reshape(N, Ho, Wo, -1)
    out = affine(xh2, p['_bn2.weight'], p['_bn2.bias'], res=x if residual else None)
    if keep is not None:
        keep.update(x=x, xh0=xh0, y0=y0, xh1=xh1, a1=a1, sum_px=sum_px, gate=gate, s=sg, xh2=xh2, se=se, wdw=wdw, Ho=Ho, Wo=Wo)
    return out


def mbconv_backward(g, p, K, k, s, pad_b, e, residual):
    """g = dL/d(out) [N, Ho, Wo, cout], K what mbconv_forward kept -> (gradients by parameter name, dL/dx)."""
    N, Ho, Wo, cout = g.shape
    H, W = K['x'].shape[1:3]
    oup = K['a1'].shape[-1]
    inv_hw = 1.0 / (Ho * Wo)
    grads = {}
    gm = g.reshape(1, -1, cout)
    db, dg, _, _ = colsums(gm, K['xh2'].reshape(1, -1, cout))
    grads['_bn2.bias'], grads['_bn2.weight'] = db[0], dg[0]
    r2, _ = bn_consts(p, '_bn2')
    f2 = p['_bn2.weight'] * r2                                      # folded into the filter rows, not into the activations
    wp = p['_project_conv.weight'][:, :, 0, 0]
    grads['_project_conv.weight'] = (f2[:, None] * (gm[0].t() @ K['s'].reshape(-1, oup)))[:, :, None, None]
    g_s = (gm[0] @ (f2[:, None] * wp)).reshape(N, Ho * Wo, oup)
    dgate = colsums(g_s, K['a1'])[1]
    sb = se_bwd(K['sum_px'], inv_hw, dgate, *K['se'])
    sq = K['se'][1].numel()
    grads['_se_reduce.weight'], grads['_se_reduce.bias'] = sb['dw1'].reshape(sq, oup, 1, 1), sb['db1']
    grads['_se_expand.weight'], grads['_se_expand.bias'] = sb['dw2'].reshape(oup, sq, 1, 1), sb['db2']
    g_y1 = swish_bwd(g_s, K['xh1'].reshape(N, Ho * Wo, oup), p['_bn1.weight'], p['_bn1.bias'], K['gate'], sb['dpool'], inv_hw)
    db, dg, _, _ = colsums(g_y1.reshape(1, -1, oup), K['xh1'].reshape(1, -1, oup))
    grads['_bn1.bias'], grads['_bn1.weight'] = db[0], dg[0]
    r1, _ = bn_consts(p, '_bn1')
    f1 = p['_bn1.weight'] * r1
    g4 = g_y1.reshape(N, Ho, Wo, oup)
    dw, _ = dw_wgrad(g4, K['y0'], k, s, pad_b, act=e != 1)
    grads['_depthwise_conv.weight'] = (dw * f1).t().reshape(oup, 1, k, k)
    g_y0 = dw_dgrad(g4, K['wdw'] * f1, H, W, k, s, pad_b, y=K['y0'] if e != 1 else None)
    if e != 1:
        cin = K['x'].shape[-1]
        gm0 = g_y0.reshape(1, -1, oup)
        db, dg, _, _ = colsums(gm0, K['xh0'].reshape(1, -1, oup))
        grads['_bn0.bias'], grads['_bn0.weight'] = db[0], dg[0]
        r0, _ = bn_consts(p, '_bn0')
        f0 = p['_bn0.weight'] * r0
        we = p['_expand_conv.weight'][:, :, 0, 0]
        grads['_expand_conv.weight'] = (f0[:, None] * (gm0[0].t() @ K['x'].reshape(-1, cin)))[:, :, None, None]
        gx = (gm0[0] @ (f0[:, None] * we)).reshape(K['x'].shape)
    else:
        gx = g_y0
    return grads, gx + g if residual else gx


def mbconv_torch(x_nchw, p, k, s, pad, e, residual):
    """The same block in torch's own operators, NCHW (what oracle/linknet_ref.encoder does per block); pad = (before, after)."""
    x = x_nchw
    bn = lambda t, n: F.batch_norm(t, p[n + '.running_mean'], p[n + '.running_var'], p[n + '.weight'], p[n + '.bias'], False, 0.0, BN_EPS_ENC)
    if e != 1:
        x = swish(bn(F.conv2d(x, p['_expand_conv.weight']), '_bn0'))
    x = F.conv2d(F.pad(x, (pad[0], pad[1], pad[0], pad[1])), p['_depthwise_conv.weight'], stride=s, groups=x.shape[1])
    x = swish(bn(x, '_bn1'))
    q = F.adaptive_avg_pool2d(x, 1)
    q = swish(F.conv2d(q, p['_se_reduce.weight'], p['_se_reduce.bias']))
    x = torch.sigmoid(F.conv2d(q, p['_se_expand.weight'], p['_se_expand.bias'])) * x
    x = bn(F.conv2d(x, p['_project_conv.weight']), '_bn2')
    return x + x_nchw if residual else x


# ------------------------------------------------------------------------------------------------ calls that must be refused
def refusals(lib, x, g, w, v, gate, img, gs, o, p, S):
    """Every bad call of the entry points around one good depthwise shape (N, H, W, C, k, stride) = (2, 6, 4, 8, 5, 2), Ho, Wo =
    3, 2, pad 1.  x [48][8], g [12][8], w [25][8], v [8], gate [2][8], img [2][3][6][4], gs [12][48] inputs, o an output of at
    least 48 x 64 floats, p scratch; -> [(what, entry, status)].  The checks run on the host before anything is launched, so
    the host test calls this with pointers that are never dereferenced."""
    N, H, W, C, k, s = 2, 6, 4, 8, 5, 2
    Ho, Wo, pb = 3, 2, 1
    Mi, Mo = N * H * W, N * Ho * Wo
    dw_ok = dict(N=N, H=H, W=W, C=C, ldg=C, ldx=C, k=k, s=s, pb=pb, Ho=Ho, Wo=Wo)
    bad = []
    for change in (dict(C=6), dict(C=0), dict(ldx=4), dict(ldg=10), dict(k=4), dict(k=7), dict(s=3), dict(s=0), dict(N=-1), dict(H=0), dict(W=-3),
                   dict(pb=-1), dict(pb=5), dict(Ho=0), dict(Wo=-2), dict(Ho=5), dict(Wo=4), dict(Ho=1 << 30)):
        a = dict(dw_ok, **change)
        geo = (a['k'], a['s'], a['pb'], a['Ho'], a['Wo'])
        bad += [(change, 'dwconv', lib.vfn_et_dwconv_f32(x, w, v, v, o, a['N'], a['H'], a['W'], a['C'], a['ldx'], a['ldg'], *geo, 1, S)),
                (change, 'dgrad', lib.vfn_et_dw_dgrad_f32(g, w, x, o, a['N'], a['H'], a['W'], a['C'], a['ldg'], a['ldx'], a['ldx'], *geo, 1, S)),
                (change, 'wgrad', lib.vfn_et_dw_wgrad_f32(g, x, p, o, a['N'], a['H'], a['W'], a['C'], a['ldg'], a['ldx'], *geo, 1, S))]
    bad += [('null', 'dwconv', lib.vfn_et_dwconv_f32(None, w, v, v, o, N, H, W, C, C, C, k, s, pb, Ho, Wo, 0, S)),
            ('null y', 'dgrad', lib.vfn_et_dw_dgrad_f32(g, w, None, o, N, H, W, C, C, C, C, k, s, pb, Ho, Wo, 1, S)),
            ('null part', 'wgrad', lib.vfn_et_dw_wgrad_f32(g, x, None, o, N, H, W, C, C, C, k, s, pb, Ho, Wo, 0, S)),
            ('C % 4', 'affine', lib.vfn_et_affine_f32(x, v, v, None, o, Mi, 6, C, C, C, 0, S)),
            ('M = 0', 'affine', lib.vfn_et_affine_f32(x, v, v, None, o, 0, C, C, C, C, 0, S)),
            ('ld_y < C', 'affine', lib.vfn_et_affine_f32(x, v, v, None, o, Mi, C, C, C, 4, 0, S)),
            ('null scale', 'affine', lib.vfn_et_affine_f32(x, None, v, None, o, Mi, C, C, C, C, 0, S)),
            ('ld_res', 'affine', lib.vfn_et_affine_f32(x, v, v, x, o, Mi, C, C, 6, C, 0, S)),
            ('B = 0', 'scale_rows', lib.vfn_et_scale_rows_f32(x, gate, o, 0, H * W, C, C, C, S)),
            ('null gate', 'scale_rows', lib.vfn_et_scale_rows_f32(x, None, o, N, H * W, C, C, C, S)),
            ('ld % 4', 'scale_rows', lib.vfn_et_scale_rows_f32(x, gate, o, N, H * W, C, C, 10, S)),
            ('B > max', 'colsums', lib.vfn_et_colsums_f32(x, None, 257, 1, C, C, C, p, o, None, S)),
            ('a without sum_ga', 'colsums', lib.vfn_et_colsums_f32(x, x, N, H * W, C, C, C, p, o, None, S)),
            ('no output', 'colsums', lib.vfn_et_colsums_f32(x, None, N, H * W, C, C, C, p, None, None, S)),
            ('M < 1', 'colsums', lib.vfn_et_colsums_f32(x, None, N, -4, C, C, C, p, o, None, S)),
            ('null part', 'colsums', lib.vfn_et_colsums_f32(x, None, N, H * W, C, C, C, None, o, None, S)),
            ('sq = 0', 'se_bwd', lib.vfn_et_se_bwd_f32(gate, 1.0, gate, w, v, w, v, o, o, o, o, o, o, N, C, 0, C, S)),
            ('sq > max', 'se_bwd', lib.vfn_et_se_bwd_f32(gate, 1.0, gate, w, v, w, v, o, o, o, o, o, o, N, C, 257, C, S)),
            ('Cpad < C', 'se_bwd', lib.vfn_et_se_bwd_f32(gate, 1.0, gate, w, v, w, v, o, o, o, o, o, o, N, C, 2, 4, S)),
            ('B = 0', 'se_bwd', lib.vfn_et_se_bwd_f32(gate, 1.0, gate, w, v, w, v, o, o, o, o, o, o, 0, C, 2, C, S)),
            ('null tmp', 'se_bwd', lib.vfn_et_se_bwd_f32(gate, 1.0, gate, w, v, w, v, None, o, o, o, o, o, N, C, 2, C, S)),
            ('gate without dpool', 'swish_bwd', lib.vfn_et_swish_bwd_f32(x, gate, None, 1.0, x, v, v, o, N, H * W, C, C, C, C, S)),
            ('C = 2', 'swish_bwd', lib.vfn_et_swish_bwd_f32(x, None, None, 1.0, x, v, v, o, N, H * W, 2, C, C, C, S)),
            ('M = 0', 'swish_bwd', lib.vfn_et_swish_bwd_f32(x, None, None, 1.0, x, v, v, o, N, 0, C, C, C, C, S)),
            ('Cp = 40', 'stem', lib.vfn_et_stem_f32(img, w, v, v, o, N, H, W, Ho, Wo, 40, 64, 0, S)),
            ('Cp % 16', 'stem', lib.vfn_et_stem_f32(img, w, v, v, o, N, H, W, Ho, Wo, 52, 64, 0, S)),
            ('ld < Cp', 'stem', lib.vfn_et_stem_f32(img, w, v, v, o, N, H, W, Ho, Wo, 64, 48, 0, S)),
            ('Ho', 'stem', lib.vfn_et_stem_f32(img, w, v, v, o, N, H, W, Ho + 1, Wo, 64, 64, 0, S)),
            ('N = 0', 'stem', lib.vfn_et_stem_f32(img, w, v, v, o, 0, H, W, Ho, Wo, 64, 64, 0, S)),
            ('Wo', 'stem_wgrad', lib.vfn_et_stem_wgrad_f32(gs, img, p, o, N, H, W, Ho, Wo + 1, 48, 0, S)),
            ('ld_g', 'stem_wgrad', lib.vfn_et_stem_wgrad_f32(gs, img, p, o, N, H, W, Ho, Wo, 44, 0, S)),
            ('null x', 'stem_wgrad', lib.vfn_et_stem_wgrad_f32(gs, None, p, o, N, H, W, Ho, Wo, 48, 0, S))]
    return bad


# ------------------------------------------------------------------------------------------- the whole passes under autograd
def encoder_names(state):
    """The 413 tensors of ``encoder.*`` that receive a gradient."""
    return [k for k in state if k.startswith('encoder.') and k.endswith(('.weight', '.bias')) and k not in UNUSED]


def encoder_reference(state, x, gtaps, dtype=torch.float64):
    """``oracle/linknet_ref.encoder`` (eval mode) in ``dtype`` under autograd, pulled back from given gradients of its five
    features: x [N, 3, H, W], gtaps five [N, C, h, w] -> (the five features, the gradients of the 413 tensors by name)."""
    from oracle import linknet_ref as O
    names = encoder_names(state)
    sd = {k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu()) for k, v in state.items()}
    for k in names:
        sd[k].requires_grad_(True)
    feats = O.encoder(sd, x.detach().cpu().to(dtype))[1:]
    total = sum((f * g.to(dtype)).sum() for f, g in zip(feats, gtaps))
    grads = torch.autograd.grad(total, [sd[k] for k in names])
    return [f.detach() for f in feats], dict(zip(names, (g.detach() for g in grads)))


def decoder_reference(model, feats, y, dtype=torch.float64):
    """tests/linknet_train_ref.decoder_reference with the features as leaves: ``copy.deepcopy(model.decoder)`` and the head in
    ``dtype``, train mode, under autograd.  feats: the five features deepest first [N, C, h, w]; y [N, 1, H, W].  -> (loss,
    gradients by state-dict name, running statistics by name, the summands' magnitudes of the transposed convolutions' bias
    gradients, the features' gradients deepest first)."""
    import linknet_train_ref as R0
    dec = copy.deepcopy(model.decoder).to('cpu').to(dtype).train()
    head = copy.deepcopy(model.segmentation_head).to('cpu').to(dtype)
    for p in list(dec.parameters()) + list(head.parameters()):
        p.requires_grad_(True)
        p.grad = None
    feats = [f.detach().to('cpu').to(dtype).requires_grad_(True) for f in feats]
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
    loss = R0.dice_loss(torch.sigmoid(head(x)), y.detach().to('cpu').to(dtype))
    loss.backward()
    grads = {'decoder.' + n: p.grad.detach() for n, p in dec.named_parameters()}
    grads.update({'segmentation_head.' + n: p.grad.detach() for n, p in head.named_parameters()})
    stats = {'decoder.' + n: b.detach().clone() for n, b in dec.named_buffers()}
    return loss.detach(), grads, stats, abs_sums, [f.grad.detach() for f in feats]
