"""``tests/encoder_train_ref.py`` against ``torch.autograd`` in float64 (CPU): every kernel formula of
include/vfn_encoder_train.h and one MBConv block's backward chained from them, in both block forms; then the public interface of
the statistics-frozen encoder training: the three values of ``freeze_encoder``, the command line's flags, the optimizer's
468 / 465 layout against ``torch.optim.Adam`` and the message of a resume across modes."""
import pytest
import torch
import torch.nn.functional as F

import encoder_train_ref as R

TOL = 1e-12
DW_SHAPES = [(1, 1, 1, 4, 5, 1, None, None), (2, 2, 3, 8, 3, 1, None, None), (1, 5, 7, 12, 5, 1, None, None), (1, 4, 6, 12, 3, 2, None, None),
             (2, 6, 4, 36, 5, 2, None, None), (1, 5, 7, 4, 3, 2, 2, 3), (1, 6, 8, 4, 3, 2, 2, 3)]


def _r(gen, *s):
    return torch.randn(*s, generator=gen, dtype=torch.float64)


def _close(a, b, what):
    scale = max(b.abs().max().item(), 1e-300)
    assert a.shape == b.shape and (a - b).abs().max().item() <= TOL * max(scale, 1.0), (what, (a - b).abs().max().item(), scale)


def _pads(k, s, H, Ho, pb):
    """(before, after) for F.pad; after may be negative (a crop)."""
    return pb, (Ho - 1) * s + k - H - pb


@pytest.mark.parametrize('shape', DW_SHAPES)
@pytest.mark.parametrize('act', [False, True])
def test_depthwise_formulas_equal_autograd(shape, act):
    from oracle.linknet_ref import same_pad
    N, H, W, C, k, s, Ho, Wo = shape
    Ho, Wo = (H // s if Ho is None else Ho), (W // s if Wo is None else Wo)
    pb = same_pad(k, s)[0]
    gen = torch.Generator().manual_seed(7)
    x, w, g = _r(gen, N, H, W, C).requires_grad_(True), _r(gen, k * k, C).requires_grad_(True), _r(gen, N, Ho, Wo, C)
    xin = (R.swish(x) if act else x).permute(0, 3, 1, 2)
    (pt, ab), (pl, ar) = _pads(k, s, H, Ho, pb), _pads(k, s, W, Wo, pb)
    out = F.conv2d(F.pad(xin, (pl, ar, pt, ab)), w.t().reshape(C, 1, k, k), stride=s, groups=C).permute(0, 2, 3, 1)
    assert out.shape == (N, Ho, Wo, C)
    _close(R.dw_forward(xin.permute(0, 2, 3, 1).detach(), w.detach(), k, s, pb, Ho, Wo), out.detach(), 'forward')
    gx, gw = torch.autograd.grad(out, (x, w), g)
    _close(R.dw_dgrad(g, w.detach(), H, W, k, s, pb, y=x.detach() if act else None), gx, 'dgrad')
    _close(R.dw_wgrad(g, x.detach(), k, s, pb, act=act)[0], gw, 'wgrad')
    if shape == (1, 6, 8, 4, 3, 2, 2, 3):
        assert not gx[:, -1].any() and not gx[:, :, -1].any() and gx[:, :-1, :-1].abs().min() > 0


def test_oracle_geometry_is_the_models():
    """Ho = H // s with the oracle's static padding is what ``dw_forward`` computes at the model's even sizes."""
    from oracle.linknet_ref import same_pad, _conv_same
    gen = torch.Generator().manual_seed(3)
    for k, s, H, W in ((3, 1, 4, 6), (5, 1, 2, 2), (3, 2, 8, 4), (5, 2, 6, 10)):
        x, w = _r(gen, 2, H, W, 8), _r(gen, k * k, 8)
        want = _conv_same(x.permute(0, 3, 1, 2), w.t().reshape(8, 1, k, k), k, s, groups=8).permute(0, 2, 3, 1)
        _close(R.dw_forward(x, w, k, s, same_pad(k, s)[0], H // s, W // s), want[:, :H // s, :W // s], (k, s))


def test_squeeze_excite_and_swish_formulas_equal_autograd():
    gen = torch.Generator().manual_seed(11)
    for B, C, sq, M in ((1, 4, 1, 3), (3, 40, 6, 5)):
        a1 = _r(gen, B, M, C).requires_grad_(True)
        xh, gamma, beta = _r(gen, B, M, C).requires_grad_(True), _r(gen, C), _r(gen, C)
        w1, b1, w2, b2 = (t.requires_grad_(True) for t in (_r(gen, sq, C), _r(gen, sq), _r(gen, C, sq), _r(gen, C)))
        # the gate from the column sums, its backward from dgate
        spx = R.colsums(a1)[0]
        gate = R.se_gate(spx, 1.0 / M, w1, b1, w2, b2)[3]
        dgate = _r(gen, B, C)
        want = torch.autograd.grad(gate, (spx, w1, b1, w2, b2), dgate, retain_graph=True)
        got = R.se_bwd(spx.detach(), 1.0 / M, dgate, w1.detach(), b1.detach(), w2.detach(), b2.detach())
        _close(got['dpool'] / M, want[0], 'dpool')               # (dpool: with respect to the MEAN)
        for k_, wv in zip(('dw1', 'db1', 'dw2', 'db2'), want[1:]):
            _close(got[k_], wv, k_)
        # s = gate(swish(y1)) swish(y1), y1 = gamma xh + beta: the whole gated activation backwards in one formula
        y1 = xh * gamma + beta
        a = R.swish(y1)
        spx2 = R.colsums(a)[0]
        gate2 = R.se_gate(spx2, 1.0 / M, w1, b1, w2, b2)[3]
        s_ = R.scale_rows(a, gate2)
        g_s = _r(gen, B, M, C)
        want_xh, = torch.autograd.grad(s_, xh, g_s)
        dg = R.colsums(g_s, a.detach())[1]
        sb = R.se_bwd(spx2.detach(), 1.0 / M, dg, w1.detach(), b1.detach(), w2.detach(), b2.detach())
        g_y1 = R.swish_bwd(g_s, xh.detach(), gamma, beta, gate2.detach(), sb['dpool'], 1.0 / M)
        _close(g_y1 * gamma, want_xh, 'g_y1')
        _close(R.swish_bwd(g_s, xh.detach(), gamma, beta), torch.autograd.grad(R.swish(xh * gamma + beta), xh, g_s)[0] / gamma, 'plain swish')


def test_stem_formulas_equal_autograd():
    from oracle.linknet_ref import same_pad, _conv_same
    gen = torch.Generator().manual_seed(5)
    for N, H, W in ((1, 2, 2), (2, 6, 10), (1, 5, 7)):
        Ho, Wo = (H + 1) // 2, (W + 1) // 2
        x, w = _r(gen, N, 3, H, W), _r(gen, 48, 3, 3, 3).requires_grad_(True)
        scale, shift, g = _r(gen, 48), _r(gen, 48), _r(gen, N, Ho, Wo, 48)
        pb = same_pad(3, 2)[0]
        conv = F.conv2d(F.pad(x, (pb, 2, pb, 2)), w, stride=2)[:, :, :Ho, :Wo].permute(0, 2, 3, 1)
        _close(R.stem_forward(x, w.detach(), scale, shift, Ho, Wo, pb), (conv * scale + shift).detach(), 'stem forward')
        _close(R.stem_wgrad(g, x, pb)[0], torch.autograd.grad(conv, w, g)[0], 'stem wgrad')
        if H % 2 == 0 and W % 2 == 0:
            _close(conv.detach(), _conv_same(x, w.detach(), 3, 2).permute(0, 2, 3, 1), 'oracle geometry')


# (cin, cout, k, s, e, residual): the first form has no expand convolution; the second has a residual; then strided 5x5
BLOCKS = [(8, 4, 3, 1, 1, False), (8, 8, 3, 1, 1, True), (4, 4, 5, 1, 6, True), (4, 8, 5, 2, 6, False), (4, 8, 3, 2, 6, False)]


@pytest.mark.parametrize('blk', BLOCKS)
def test_block_backward_chained_from_the_formulas_equals_autograd(blk):
    from oracle.linknet_ref import same_pad
    cin, cout, k, s, e, residual = blk
    gen = torch.Generator().manual_seed(21)
    N, H, W = 2, 4, 6
    p = {n: v.requires_grad_(not n.endswith(('running_mean', 'running_var'))) for n, v in R.mbconv_params(cin, cout, k, e, max(1, cin // 4), gen).items()}
    x = _r(gen, N, H, W, cin).requires_grad_(True)
    out = R.mbconv_torch(x.permute(0, 3, 1, 2), p, k, s, same_pad(k, s), e, residual).permute(0, 2, 3, 1)
    g = _r(gen, *out.shape)
    names = [n for n, v in p.items() if v.requires_grad]
    want = torch.autograd.grad(out, [x] + [p[n] for n in names], g)
    with torch.no_grad():
        keep = {}
        mine = R.mbconv_forward(x.detach(), p, k, s, same_pad(k, s)[0], e, residual, keep=keep)
        _close(mine, out.detach(), 'forward')
        grads, gx = R.mbconv_backward(g, p, keep, k, s, same_pad(k, s)[0], e, residual)
    _close(gx, want[0], 'gx')
    assert sorted(grads) == sorted(names)
    for n, wv in zip(names, want[1:]):
        _close(grads[n], wv, n)


def test_bad_arguments_are_refused_before_any_launch():
    """The entry points check their arguments on the host: with pointers that are never dereferenced every bad call comes back
    as VFN_ERR_ARG (1) without a device."""
    import ctypes
    from vfloodnet_amd import _lib
    L = _lib.lib()
    P = ctypes.c_void_p(4096)
    bad = R.refusals(L, P, P, P, P, P, P, P, P, P, None)
    assert len(bad) > 80 and all(st == 1 for _, _, st in bad), [b for b in bad if b[2] != 1]


# ------------------------------------------------------------------------------------------------------- the interface
def test_freeze_encoder_has_three_values():
    from vfloodnet_amd import train_image_seg as T
    from vfloodnet_amd.linknet import LinknetB4
    from vfloodnet_amd.linknet_train import ENCODER_MISSING, freeze_encoder, freeze_encoder_statistics
    for word in ('BatchNorm', 'drop-connect', 'depthwise', 'squeeze-excite', "freeze_encoder='statistics'"):
        assert word in ENCODER_MISSING
    for bad in (False, None, 0):
        with pytest.raises(NotImplementedError, match='drop-connect'):
            T.TrainEpoch(None, 'cuda', freeze_encoder=bad)
        with pytest.raises(NotImplementedError, match='train mode'):
            T.train_model(None, 1e-4, 1, '.', None, None, freeze_encoder=bad)
    with pytest.raises(ValueError, match="'statistics'"):
        T.TrainEpoch(None, 'cuda', freeze_encoder='stats')
    for mode in (True, 'statistics'):                          # both pass the mode check and stop at the device: no CPU fallback
        with pytest.raises(RuntimeError, match='GPU only'):
            T.TrainEpoch(None, 'cpu', freeze_encoder=mode)
    model = LinknetB4()
    assert freeze_encoder_statistics(model) is model and model.training and not model.encoder.training and model.decoder.training
    assert all(p.requires_grad for p in model.parameters())
    freeze_encoder(model)
    assert sum(p.requires_grad for p in model.parameters()) == 52
    freeze_encoder_statistics(model)
    assert sum(p.requires_grad for p in model.parameters()) == 468


def test_command_line_flags():
    from vfloodnet_amd import train_image_seg as T
    base = ['--dataset-path', 'x', '--model-path', 'y']
    a = T.get_args(base + ['--freeze-encoder-statistics'])
    assert a.freeze_encoder_statistics and not a.freeze_encoder
    a = T.get_args(base + ['--freeze-encoder'])
    assert a.freeze_encoder and not a.freeze_encoder_statistics
    with pytest.raises(SystemExit):                            # mutually exclusive
        T.get_args(base + ['--freeze-encoder', '--freeze-encoder-statistics'])
    with pytest.raises(NotImplementedError, match='--freeze-encoder-statistics'):
        T.main(base)
    with pytest.raises(ValueError, match='efficientnet-b4'):   # the flag alone passes the mode check
        T.main(base + ['--encoder', 'resnet34', '--freeze-encoder-statistics'])


def _host_adam(model, skip):
    """``linknet_train.Adam`` with its buffers on the CPU: the constructor insists on the GPU (there is no CPU step), the state
    dict's layout is plain bookkeeping."""
    from vfloodnet_amd.linknet_train import Adam
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    opt = Adam.__new__(Adam)
    opt.lr, opt.betas, opt.eps, opt.weight_decay, opt.initial_lr, opt.step_count = 1e-3, (0.9, 0.999), 1e-8, 0.0, None, 0
    opt.names, opt.offsets, off = [n for n, _ in named if n not in skip], {}, 0
    for n, p in named:
        if n not in skip:
            opt.offsets[n] = (off, p.numel(), tuple(p.shape))
            off += (p.numel() + 3) // 4 * 4
    opt.exp_avg, opt.exp_avg_sq = torch.zeros(off), torch.zeros(off)
    opt.n_group, opt.index = len(named), [i for i, (n, _) in enumerate(named) if n not in skip]
    return opt


def test_optimizer_layout_is_torch_adams_over_468_parameters():
    """``state_dict()`` numbers all 468 parameters in ``model.parameters()`` order and holds state for the 465 that receive a
    gradient: ``torch.optim.Adam(model.parameters())`` on a CPU copy loads it, and its own state dict loads back."""
    from vfloodnet_amd import train_image_seg as T
    from vfloodnet_amd.linknet import LinknetB4
    from vfloodnet_amd.linknet_train import UNUSED, freeze_encoder, freeze_encoder_statistics
    model = freeze_encoder_statistics(LinknetB4())
    everyone = [n for n, _ in model.named_parameters()]
    assert len(everyone) == 468 and all(n in everyone for n in UNUSED) and UNUSED == R.UNUSED
    opt = _host_adam(model, UNUSED)
    assert len(opt.names) == 465
    opt.step_count = 3
    opt.exp_avg.normal_()
    opt.exp_avg_sq.uniform_()
    sd = opt.state_dict()
    topt = torch.optim.Adam([dict(params=model.parameters(), lr=1e-3)])
    assert sd['param_groups'][0] == topt.state_dict()['param_groups'][0] and sd['param_groups'][0]['params'] == list(range(468))
    assert sorted(sd['state']) == [i for i, n in enumerate(everyone) if n not in UNUSED]
    topt.load_state_dict(sd)
    # torch's own step gives the same layout: the three unused tensors have no gradient, so no state
    for n, p in model.named_parameters():
        p.grad = None if n in UNUSED else torch.zeros_like(p)
    topt.step()
    back = topt.state_dict()
    assert sorted(back['state']) == sorted(sd['state']) and float(back['state'][0]['step']) == 4.0
    other = _host_adam(model, UNUSED)
    other.load_state_dict(back)
    assert other.step_count == 4 and other.exp_avg.abs().sum() > 0
    i = everyone.index('decoder.blocks.0.block.0.0.weight')
    o, k, shp = other.offsets['decoder.blocks.0.block.0.0.weight']
    assert torch.equal(other.exp_avg[o:o + k].view(shp), back['state'][i]['exp_avg'])
    # a resume across the modes says so
    with pytest.raises(ValueError, match=r'freeze_encoder=True \(--freeze-encoder\)'):
        T.load_optimizer_state(_host_adam(freeze_encoder(LinknetB4()), ()), sd, True)
    small = _host_adam(freeze_encoder(LinknetB4()), ())
    assert small.n_group == 52 and small.index == list(range(52))
    with pytest.raises(ValueError, match='freeze-encoder-statistics'):
        T.load_optimizer_state(opt, small.state_dict(), 'statistics')
    with pytest.raises(ValueError, match='468'):
        small.load_state_dict(sd)                              # (and the optimizer itself: a message, not a shape error)
