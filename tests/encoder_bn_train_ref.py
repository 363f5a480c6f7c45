"""Restatements, in plain torch on the CPU, of what ``csrc/encoder_bn_train.hip`` and ``linknet_train.FullTrainer`` compute
(include/vfn_encoder_bn_train.h): the formulas of one batch-statistics BatchNorm in any dtype -- float64 is the reference,
float32 the yardstick of the error rule --, the drop-connect scale rule, one MBConv block in train mode chained from them the
way the product chains it, and the whole encoder in train mode under ``torch.autograd`` with a given table of drop-connect
scales.  ``tests/test_encoder_bn_train_ref_host.py`` holds every function here against ``torch.autograd`` and
``nn.BatchNorm2d``.  Activations are NHWC: [N, H, W, C], or [B, M, C] where only rows matter."""
import functools

import torch
import torch.nn.functional as F

import encoder_train_ref as R

BN_EPS_ENC = 1e-3
BN_MOMENTUM_ENC = 0.01                                          # efficientnet_pytorch: 1 - batch_norm_momentum (0.99)
DROP_CONNECT_RATE = 0.2
FACTOR = 8.0
CAP = 1e-4                                                      # a float32 reference further than this from float64: ill-conditioned input
BATCHES = [(2, 64, 64), (3, 64, 96)]
TAP_CHANNELS = R.TAP_CHANNELS


# --------------------------------------------------------------------------------------------------- the kernel formulas
def bn_stats(z, gamma, eps=BN_EPS_ENC, momentum=BN_MOMENTUM_ENC, running_mean=None, running_var=None):
    """z [M, C] -> dict(mean, var (biased), rstd, nshift, fold, and the moved running statistics when given)."""
    M = z.shape[0]
    mean = z.mean(0)
    var = ((z - mean) ** 2).mean(0)
    rstd = 1 / torch.sqrt(var + eps)
    out = dict(mean=mean, var=var, rstd=rstd, nshift=-mean * rstd, fold=gamma * rstd)
    if running_mean is not None:
        out['running_mean'] = (1 - momentum) * running_mean + momentum * mean
        out['running_var'] = (1 - momentum) * running_var + momentum * var * M / (M - 1)
    return out


def bn_norm(z, rstd, nshift, gamma, beta, keep=None, res=None, act=False):
    """z [B, M, C], keep [B] -> (xh, y)."""
    xh = z * rstd + nshift
    y = xh * gamma + beta
    if act:
        y = R.swish(y)
    if keep is not None:
        y = y * keep[:, None, None]
    return xh, (y if res is None else y + res)


def bn_sums(sum_g, sum_ga, keep=None):
    """[B, C] each -> (dbeta, dgamma) [C]."""
    k = torch.ones(sum_g.shape[0], dtype=sum_g.dtype) if keep is None else keep
    return (sum_g * k[:, None]).sum(0), (sum_ga * k[:, None]).sum(0)


def bn_center(g, xh, dbeta, dgamma, keep=None):
    """g, xh [B, M, C] -> g' = keep g - dbeta / (B M) - xh dgamma / (B M)."""
    rows = g.shape[0] * g.shape[1]
    kg = g if keep is None else g * keep[:, None, None]
    return kg - dbeta / rows - xh * dgamma / rows


def bn_backward(g, xh, keep=None):
    """The chain the product runs: per-image column sums, the sums under the scale, the centring -> (dbeta, dgamma, g')."""
    sg, sga, _, _ = R.colsums(g, xh)
    dbeta, dgamma = bn_sums(sg, sga, keep)
    return dbeta, dgamma, bn_center(g, xh, dbeta, dgamma, keep)


# -------------------------------------------------------------------------------------------------------- drop-connect
def drop_connect_rates():
    """[(block index, rate)] of the blocks under drop-connect: residual (stride 1, cin == cout) with rate 0.2 i / 32 > 0."""
    from oracle import linknet_ref as O
    blocks = O.blocks()
    return [(i, DROP_CONNECT_RATE * i / len(blocks)) for i, b in enumerate(blocks) if b['s'] == 1 and b['cin'] == b['cout'] and i > 0]


def keep_scale(u, p):
    """efficientnet_pytorch's drop_connect: the factor of an image's branch, floor(1 - p + u) / (1 - p)."""
    return torch.floor(1 - p + u) / (1 - p)


def tests_keep(N):
    """The table the tests pass, [blocks under drop-connect][N] float32: rows 4 and 20 drop image 0, row 13 drops image 1; every
    other entry is 1 / (1 - p).  (The host test holds the float32 reference under this table to ``CAP``; at batch (2, 64, 64)
    other tables were measured between 5e-5 and 1.6e-4, this one at 5.2e-5.)"""
    rates = drop_connect_rates()
    t = torch.stack([torch.full((N,), 1 / (1 - p), dtype=torch.float64) for _, p in rates])
    for r, n in TESTS_DROPS:
        t[r, n] = 0.0
    return t.float()


TESTS_DROPS = ((4, 0), (13, 1), (20, 0))                        # (row of the table, image)


# ----------------------------------------------------------------------------- one MBConv block in train mode, chained as the product
def mbconv_train_forward(x, p, k, s, pad_b, e, residual, keep_n=None, kept=None):
    """``encoder_train_ref.mbconv_forward`` with batch statistics: each convolution leaves its raw output, the statistics follow,
    then the normalisation; ``keep_n`` [N]: the block's drop-connect scales."""
    N, H, W, _ = x.shape
    Ho, Wo = H // s, W // s
    K = dict(x=x, Ho=Ho, Wo=Wo)

    def bn(z, name, act=False, keep=None, res=None):
        C = z.shape[-1]
        st = bn_stats(z.reshape(-1, C), p[name + '.weight'])
        xh, y = bn_norm(z.reshape(N, -1, C), st['rstd'], st['nshift'], p[name + '.weight'], p[name + '.bias'], keep,
                        None if res is None else res.reshape(N, -1, C), act)
        K['fold' + name[-1]] = st['fold']
        return xh.reshape(z.shape), y.reshape(z.shape)

    if e != 1:
        K['xh0'], K['y0'] = bn(x @ p['_expand_conv.weight'][:, :, 0, 0].t(), '_bn0')
    else:
        K['xh0'], K['y0'] = None, x
    oup = K['y0'].shape[-1]
    K['wdw'] = p['_depthwise_conv.weight'].reshape(oup, k * k).t()
    K['xh1'], a1 = bn(R.dw_forward(R.swish(K['y0']) if e != 1 else K['y0'], K['wdw'], k, s, pad_b, Ho, Wo), '_bn1', act=True)
    K['a1'] = a1.reshape(N, Ho * Wo, oup)
    sq = p['_se_reduce.bias'].numel()
    K['sum_px'] = R.colsums(K['a1'])[0]
    K['se'] = (p['_se_reduce.weight'].reshape(sq, oup), p['_se_reduce.bias'], p['_se_expand.weight'].reshape(oup, sq), p['_se_expand.bias'])
    K['gate'] = R.se_gate(K['sum_px'], 1.0 / (Ho * Wo), *K['se'])[3]
    K['s'] = R.scale_rows(K['a1'], K['gate'])
    K['xh2'], out = bn((K['s'] @ p['_project_conv.weight'][:, :, 0, 0].t()).reshape(N, Ho, Wo, -1), '_bn2', keep=keep_n, res=x if residual else None)
    if kept is not None:
        kept.update(K)
    return out


def mbconv_train_backward(g, p, K, k, s, pad_b, e, residual, keep_n=None):
    """g = dL/d(out) -> (gradients by parameter name, dL/dx): ``encoder_train_ref.mbconv_backward`` with the centring behind each
    pair of column sums and gamma (batch rstd) as the fold."""
    N, Ho, Wo, cout = g.shape
    H, W = K['x'].shape[1:3]
    oup = K['a1'].shape[-1]
    inv_hw = 1.0 / (Ho * Wo)
    grads = {}
    grads['_bn2.bias'], grads['_bn2.weight'], gc = bn_backward(g.reshape(N, -1, cout), K['xh2'].reshape(N, -1, cout), keep_n)
    gm = gc.reshape(-1, cout)
    wp = p['_project_conv.weight'][:, :, 0, 0]
    grads['_project_conv.weight'] = (K['fold2'][:, None] * (gm.t() @ K['s'].reshape(-1, oup)))[:, :, None, None]
    g_s = (gm @ (K['fold2'][:, None] * wp)).reshape(N, Ho * Wo, oup)
    dgate = R.colsums(g_s, K['a1'])[1]
    sb = R.se_bwd(K['sum_px'], inv_hw, dgate, *K['se'])
    sq = K['se'][1].numel()
    grads['_se_reduce.weight'], grads['_se_reduce.bias'] = sb['dw1'].reshape(sq, oup, 1, 1), sb['db1']
    grads['_se_expand.weight'], grads['_se_expand.bias'] = sb['dw2'].reshape(oup, sq, 1, 1), sb['db2']
    g_y1 = R.swish_bwd(g_s, K['xh1'].reshape(N, Ho * Wo, oup), p['_bn1.weight'], p['_bn1.bias'], K['gate'], sb['dpool'], inv_hw)
    grads['_bn1.bias'], grads['_bn1.weight'], g1 = bn_backward(g_y1, K['xh1'].reshape(N, -1, oup))
    g4 = g1.reshape(N, Ho, Wo, oup)
    dw, _ = R.dw_wgrad(g4, K['y0'], k, s, pad_b, act=e != 1)
    grads['_depthwise_conv.weight'] = (dw * K['fold1']).t().reshape(oup, 1, k, k)
    g_y0 = R.dw_dgrad(g4, K['wdw'] * K['fold1'], H, W, k, s, pad_b, y=K['y0'] if e != 1 else None)
    if e != 1:
        cin = K['x'].shape[-1]
        grads['_bn0.bias'], grads['_bn0.weight'], g0 = bn_backward(g_y0.reshape(N, -1, oup), K['xh0'].reshape(N, -1, oup))
        gm0 = g0.reshape(-1, oup)
        we = p['_expand_conv.weight'][:, :, 0, 0]
        grads['_expand_conv.weight'] = (K['fold0'][:, None] * (gm0.t() @ K['x'].reshape(-1, cin)))[:, :, None, None]
        gx = (gm0 @ (K['fold0'][:, None] * we)).reshape(K['x'].shape)
    else:
        gx = g_y0
    return grads, gx + g if residual else gx


def mbconv_train_torch(x_nchw, p, k, s, pad, e, residual, keep_n=None):
    """The same block in torch's own operators, NCHW, ``F.batch_norm(training=True)``; pad = (before, after)."""
    x = x_nchw
    bn = lambda t, n: F.batch_norm(t, None, None, p[n + '.weight'], p[n + '.bias'], True, BN_MOMENTUM_ENC, BN_EPS_ENC)
    if e != 1:
        x = R.swish(bn(F.conv2d(x, p['_expand_conv.weight']), '_bn0'))
    x = F.conv2d(F.pad(x, (pad[0], pad[1], pad[0], pad[1])), p['_depthwise_conv.weight'], stride=s, groups=x.shape[1])
    x = R.swish(bn(x, '_bn1'))
    q = F.adaptive_avg_pool2d(x, 1)
    q = R.swish(F.conv2d(q, p['_se_reduce.weight'], p['_se_reduce.bias']))
    x = torch.sigmoid(F.conv2d(q, p['_se_expand.weight'], p['_se_expand.bias'])) * x
    x = bn(F.conv2d(x, p['_project_conv.weight']), '_bn2')
    if keep_n is not None:
        x = x * keep_n[:, None, None, None]
    return x + x_nchw if residual else x


# ------------------------------------------------------------------------------------------- the whole encoder in train mode
def encoder_train(sd, x, keep):
    """``oracle/linknet_ref.encoder`` in train mode: every BatchNorm through ``F.batch_norm(training=True)`` (momentum 0.01), which
    moves ``sd``'s running statistics in place, and the residual blocks under the scales ``keep`` [blocks under drop-connect][N].
    -> the five features smp's encoder returns behind its input."""
    from oracle import linknet_ref as O
    rows = {i: r for r, (i, _) in enumerate(drop_connect_rates())}

    def bn(t, prefix):
        return F.batch_norm(t, sd[prefix + '.running_mean'], sd[prefix + '.running_var'], sd[prefix + '.weight'], sd[prefix + '.bias'], True,
                            BN_MOMENTUM_ENC, BN_EPS_ENC)

    x = R.swish(bn(O._conv_same(x, sd['encoder._conv_stem.weight'], 3, 2), 'encoder._bn0'))
    feats = [x]
    for i, b in enumerate(O.blocks()):
        p = f'encoder._blocks.{i}'
        inp, oup = x, b['cin'] * b['e']
        if b['e'] != 1:
            x = R.swish(bn(F.conv2d(x, sd[p + '._expand_conv.weight']), p + '._bn0'))
        x = R.swish(bn(O._conv_same(x, sd[p + '._depthwise_conv.weight'], b['k'], b['s'], groups=oup), p + '._bn1'))
        g = F.adaptive_avg_pool2d(x, 1)
        g = R.swish(F.conv2d(g, sd[p + '._se_reduce.weight'], sd[p + '._se_reduce.bias']))
        x = torch.sigmoid(F.conv2d(g, sd[p + '._se_expand.weight'], sd[p + '._se_expand.bias'])) * x
        x = bn(F.conv2d(x, sd[p + '._project_conv.weight']), p + '._bn2')
        if b['s'] == 1 and b['cin'] == b['cout']:
            if i in rows:
                x = x * keep[rows[i]].to(x.dtype)[:, None, None, None]
            x = x + inp
        if i + 1 in O.STAGE_IDXS:
            feats.append(x)
    return feats


def stat_names(state):
    """The 190 running statistics of the encoder's 95 BatchNorms that run (encoder._bn1 belongs to the unused head)."""
    return [k for k in state if k.startswith('encoder.') and k.endswith(('running_mean', 'running_var')) and not k.startswith('encoder._bn1.')]


def encoder_train_reference(state, x, gtaps, keep, dtype=torch.float64):
    """The encoder in train mode in ``dtype`` under autograd, pulled back from given gradients of its five features: x [N, 3, H, W],
    gtaps five [N, C, h, w], keep the scale table -> (the five features, the gradients of the 413 tensors by name, the 190 moved
    running statistics by name)."""
    names = R.encoder_names(state)
    sd = {k: (v.detach().cpu().to(dtype).clone() if v.is_floating_point() else v.detach().cpu().clone()) for k, v in state.items()}
    for k in names:
        sd[k].requires_grad_(True)
    feats = encoder_train(sd, x.detach().cpu().to(dtype), keep.cpu())
    total = sum((f * g.to(dtype)).sum() for f, g in zip(feats, gtaps))
    grads = torch.autograd.grad(total, [sd[k] for k in names])
    return [f.detach() for f in feats], dict(zip(names, (g.detach() for g in grads))), {k: sd[k] for k in stat_names(state)}


def tap_gradients(N, H, W):
    """Seeded normal / sqrt(C) gradients of the five taps, NCHW."""
    gen = torch.Generator().manual_seed(1000 + H + W)
    return [torch.randn(N, c, H >> (i + 1), W >> (i + 1), generator=gen) / c ** 0.5 for i, c in enumerate(TAP_CHANNELS)]


@functools.lru_cache(maxsize=None)
def reference_pass(batch):
    """The float64 and float32 references of one batch of ``BATCHES`` on the synthetic checkpoint under ``tests_keep``: computed
    once per session, shared by the host test (which holds the cap) and the device tests, and left unchanged."""
    from tools import synth_linknet
    from test_image_train_gpu import make_batch
    N, H, W = batch
    state = synth_linknet.make_state_dict()
    x = make_batch(N, H, W)[0]
    gt, keep = tap_gradients(N, H, W), tests_keep(N)
    return dict(x=x, gt=gt, keep=keep, ref=encoder_train_reference(state, x, gt, keep), r32=encoder_train_reference(state, x, gt, keep, torch.float32))


def kind(name):
    """Tensors of a kind share a scale: the last two components of the name ('_bn2.bias')."""
    return '.'.join(name.split('.')[-2:])


def kind_scales(ref):
    """name -> the largest |ref|max over the tensors of its kind.  In train mode a bias whose only consumers are convolution ->
    batch-statistics BatchNorm (most ``_bn2.bias``) has a gradient that is zero up to rounding: its own |ref|max measures nothing."""
    top = {}
    for n, v in ref.items():
        top[kind(n)] = max(top.get(kind(n), 0.0), v.abs().max().item())
    return {n: top[kind(n)] for n in ref}


def distances(got, ref, scales):
    """name -> max |got - ref| in units of the kind's scale (inf for a NaN)."""
    out = {}
    for n, want in ref.items():
        d = (got[n].detach().cpu().double() - want.double()).abs().max().item()
        out[n] = float('inf') if d != d else d / scales[n]
    return out


# ------------------------------------------------------------------------------------------------ calls that must be refused
def refusals(lib, x, v, k, o, p, S):
    """Every bad call of the four entry points around one good shape (B, M, C, ld) = (2, 6, 8, 12).  x [12][12] input, v [8]
    a per-channel vector, k [2] the scales, o an output of at least 12 x 12 floats, p scratch; -> [(what, entry, status)].  The
    checks run on the host before anything is launched, so the host test calls this with pointers that are never dereferenced
    (o and x distinct there)."""
    B, M, C, ld = 2, 6, 8, 12
    R_ = B * M
    st = lambda **a: lib.vfn_et_bn_stats_f32(a.get('z', x), a.get('M', R_), a.get('C', C), a.get('ld', ld), a.get('gamma', v), a.get('eps', 1e-3),
                                             a.get('mom', 0.01), a.get('part', p), a.get('rstd', o), a.get('nshift', o), a.get('fold', o),
                                             a.get('rm', None), a.get('rv', None), a.get('c_run', 0), S)
    no = lambda **a: lib.vfn_et_bn_norm_f32(a.get('z', x), a.get('rstd', v), v, v, a.get('beta', v), a.get('keep', k), a.get('res', None),
                                            a.get('xh', x), a.get('y', o), a.get('B', B), a.get('M', M), a.get('C', C), a.get('ld_z', ld),
                                            a.get('ld_res', ld), a.get('ld_xh', ld), a.get('ld_y', ld), 0, S)
    su = lambda **a: lib.vfn_et_bn_sums_f32(a.get('sg', x), a.get('sga', x), k, a.get('db', o), a.get('dg', o), a.get('B', B), a.get('C', C), S)
    ce = lambda **a: lib.vfn_et_bn_center_f32(a.get('g', x), a.get('xh', x), a.get('keep', k), a.get('db', v), v, a.get('gp', o), a.get('B', B),
                                              a.get('M', M), a.get('C', C), a.get('ld_g', ld), a.get('ld_xh', ld), a.get('ld_gp', ld), S)
    bad = []
    for change in (dict(M=1), dict(M=0), dict(M=-3), dict(C=6), dict(C=0), dict(C=2), dict(ld=4), dict(ld=10), dict(z=None), dict(gamma=None),
                   dict(part=None), dict(rstd=None), dict(nshift=None), dict(fold=None), dict(rm=v), dict(rv=v), dict(rm=v, rv=v, c_run=9),
                   dict(c_run=-1), dict(eps=0.0), dict(eps=-1.0), dict(mom=1.5), dict(mom=-0.1), dict(M=1 << 30, ld=8)):
        bad.append((change, 'stats', st(**change)))
    for change in (dict(B=0), dict(M=0), dict(C=6), dict(C=0), dict(ld_z=4), dict(ld_xh=10), dict(ld_y=6), dict(res=x, ld_res=6), dict(z=None),
                   dict(rstd=None), dict(beta=None), dict(xh=None), dict(y=None), dict(xh=x, ld_xh=16), dict(y=x), dict(xh=o, y=o)):
        bad.append((change, 'norm', no(**change)))
    for change in (dict(B=0), dict(C=0), dict(sg=None), dict(sga=None), dict(db=None), dict(dg=None)):
        bad.append((change, 'sums', su(**change)))
    for change in (dict(B=0), dict(M=-1), dict(C=6), dict(C=2), dict(ld_g=4), dict(ld_xh=10), dict(ld_gp=6), dict(g=None), dict(xh=None),
                   dict(db=None), dict(gp=None), dict(gp=x), dict(gp=x, keep=None, ld_gp=16), dict(g=o, xh=x, gp=x, keep=None)):
        bad.append((change, 'center', ce(**change)))
    return bad
