"""``tests/encoder_bn_train_ref.py`` against ``torch.autograd`` and ``nn.BatchNorm2d`` in float64 (CPU): the formulas of one
batch-statistics BatchNorm (include/vfn_encoder_bn_train.h), the running-statistics rule, the drop-connect scale rule and the
blocks that carry it, one MBConv block in train mode chained from the formulas in both block forms with a dropped image; the
public interface of ``freeze_encoder='train'``; and the conditioning of the inputs the device tests use: the float32 reference
under the tests' drop-connect table stays within the cap of the error rule."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import encoder_bn_train_ref as B
import encoder_train_ref as R

TOL = 1e-11


def _r(gen, *s):
    return torch.randn(*s, generator=gen, dtype=torch.float64)


def _close(a, b, what, tol=TOL):
    scale = max(b.abs().max().item(), 1.0)
    assert a.shape == b.shape and (a - b).abs().max().item() <= tol * scale, (what, (a - b).abs().max().item(), scale)


# ------------------------------------------------------------------------------------------------------- the formulas
@pytest.mark.parametrize('shape', [(1, 2, 4), (2, 5, 8), (3, 7, 12)])
@pytest.mark.parametrize('dropped', [False, True])
def test_batchnorm_formulas_equal_autograd(shape, dropped):
    """Forward and backward of y = act(BN(z)) keep[b] + res through ``F.batch_norm(training=True)``: the statistics, xhat, y, dbeta,
    dgamma and g_z = fold g'."""
    Bn, M, C = shape
    gen = torch.Generator().manual_seed(31)
    z, gamma, beta = (3 + 2 * _r(gen, Bn, M, C)).requires_grad_(True), (1 + 0.3 * _r(gen, C)).requires_grad_(True), _r(gen, C).requires_grad_(True)
    res, g = _r(gen, Bn, M, C), _r(gen, Bn, M, C)
    keep = None
    if dropped:
        keep = torch.full((Bn,), 1.25, dtype=torch.float64)
        keep[0] = 0.0
    for act in (False, True):
        bn = F.batch_norm(z.reshape(-1, C), None, None, gamma, beta, True, 0.01, B.BN_EPS_ENC).reshape(Bn, M, C)
        y = R.swish(bn) if act else bn
        if keep is not None:
            y = y * keep[:, None, None]
        y = y + res
        want_z, want_gamma, want_beta = torch.autograd.grad(y, (z, gamma, beta), g)
        with torch.no_grad():
            st = B.bn_stats(z.reshape(-1, C), gamma)
            xh, mine = B.bn_norm(z, st['rstd'], st['nshift'], gamma, beta, keep, res, act)
            _close(mine, y, 'forward')
            # the gradient that reaches the BatchNorm's output: the scale, then the activation
            gy = g if keep is None else g * keep[:, None, None]
            if act:
                gy = gy * R.dswish(xh * gamma + beta)
            dbeta, dgamma, gc = B.bn_backward(gy, xh)
            _close(dbeta, want_beta, 'dbeta')
            _close(dgamma, want_gamma, 'dgamma')
            _close(st['fold'] * gc, want_z, 'g_z')
            if not act:                                           # the scale inside the sums and the centring, as the project BatchNorm has it
                dbeta, dgamma, gc = B.bn_backward(g, xh, keep)
                _close(dbeta, want_beta, 'dbeta under keep')
                _close(dgamma, want_gamma, 'dgamma under keep')
                _close(st['fold'] * gc, want_z, 'g_z under keep')


def test_running_statistics_follow_nn_batchnorm():
    """mean, M / (M - 1) times the biased variance, momentum 0.01, the counter; one value per channel is torch's ValueError."""
    gen = torch.Generator().manual_seed(5)
    m = torch.nn.BatchNorm2d(6, eps=1e-3, momentum=0.01).double().train()
    with torch.no_grad():
        m.running_mean.copy_(_r(gen, 6))
        m.running_var.copy_(0.5 + torch.rand(6, generator=gen, dtype=torch.float64))
        m.weight.copy_(1 + 0.2 * _r(gen, 6))
    rm, rv = m.running_mean.clone(), m.running_var.clone()
    for step, (N, h, w) in enumerate(((2, 3, 5), (1, 1, 2))):
        x = 2 + 3 * _r(gen, N, 6, h, w)
        with torch.no_grad():
            y = m(x)
        st = B.bn_stats(x.permute(0, 2, 3, 1).reshape(-1, 6), m.weight.detach(), running_mean=rm, running_var=rv)
        rm, rv = st['running_mean'], st['running_var']
        _close(rm, m.running_mean, 'running_mean')
        _close(rv, m.running_var, 'running_var')
        _close(B.bn_norm(x.permute(0, 2, 3, 1).reshape(N, -1, 6), st['rstd'], st['nshift'], m.weight.detach(), m.bias.detach())[1],
               y.permute(0, 2, 3, 1).reshape(N, -1, 6), 'y')
        assert int(m.num_batches_tracked) == step + 1
    with pytest.raises(ValueError, match='more than 1 value per channel'):
        m(_r(gen, 1, 6, 1, 1))
    # a constant channel: variance 0 exactly, rstd = 1 / sqrt(eps)
    st = B.bn_stats(torch.full((5, 4), 7.25, dtype=torch.float64), torch.ones(4, dtype=torch.float64))
    assert not st['var'].any() and torch.equal(st['rstd'], torch.full((4,), 1e-3, dtype=torch.float64).rsqrt())


def test_encoder_batchnorms_carry_the_reference_momentum():
    from vfloodnet_amd.linknet import LinknetB4
    model = LinknetB4()
    enc = [m for m in model.encoder.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    dec = [m for m in model.decoder.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(enc) == 96 and all(m.momentum == B.BN_MOMENTUM_ENC and m.eps == B.BN_EPS_ENC for m in enc)
    assert len(dec) == 15 and all(m.momentum == 0.1 and m.eps == 1e-5 for m in dec)


# ------------------------------------------------------------------------------------------------------- drop-connect
def test_drop_connect_scale_rule_and_its_blocks():
    from oracle import linknet_ref as O
    from vfloodnet_amd import linknet_train as T
    rates = B.drop_connect_rates()
    blocks = O.blocks()
    assert len(rates) == 25 and T.drop_connect_rates() == rates
    firsts = {0, 2, 6, 10, 16, 22, 30}                           # the first block of each of the seven stages changes shape: no residual
    assert [i for i, _ in rates] == [i for i in range(32) if i not in firsts]
    assert all(blocks[i]['s'] == 1 and blocks[i]['cin'] == blocks[i]['cout'] and p == 0.2 * i / 32 for i, p in rates)
    assert rates[0] == (1, 0.2 / 32) and rates[-1] == (31, 0.2 * 31 / 32)
    gen = torch.Generator().manual_seed(9)
    u = torch.rand(25, 64, generator=gen, dtype=torch.float64)
    u[:, 0], u[:, 1] = 0.0, 1.0 - 2.0 ** -53                    # the ends of [0, 1)
    p = torch.tensor([r for _, r in rates], dtype=torch.float64)[:, None]
    k = B.keep_scale(u, p)
    assert torch.equal(k == 0, u < p) and torch.equal(k[k != 0], (1 / (1 - p)).expand_as(k)[k != 0])
    assert not k[:, 0].any() and k[:, 1].all()
    assert torch.equal(T.keep_table(u), k.float())
    with pytest.raises(ValueError, match='one row of draws per block'):
        T.keep_table(u[:24])
    t = B.tests_keep(3)
    assert t.shape == (25, 3) and int((t == 0).sum()) == 3 and all(t[r, n] == 0 for r, n in B.TESTS_DROPS)
    assert (t == 0).any(1).sum() == 3 and (t != 0).any(1).all()


# (cin, cout, k, s, e, residual): without an expand convolution and with one; residual blocks are the ones under drop-connect
BLOCKS = [(8, 4, 3, 1, 1, False), (8, 8, 3, 1, 1, True), (4, 4, 5, 1, 6, True), (4, 8, 5, 2, 6, False)]


@pytest.mark.parametrize('blk', BLOCKS)
def test_train_mode_block_chained_from_the_formulas_equals_autograd(blk):
    from oracle.linknet_ref import same_pad
    cin, cout, k, s, e, residual = blk
    gen = torch.Generator().manual_seed(23)
    N, H, W = 3, 4, 6
    p = {n: v.requires_grad_(True) for n, v in R.mbconv_params(cin, cout, k, e, max(1, cin // 4), gen).items() if 'running' not in n}
    x = _r(gen, N, H, W, cin).requires_grad_(True)
    keep = torch.tensor([1 / 0.9, 0.0, 1 / 0.9], dtype=torch.float64) if residual else None      # the middle image is dropped
    out = B.mbconv_train_torch(x.permute(0, 3, 1, 2), p, k, s, same_pad(k, s), e, residual, keep).permute(0, 2, 3, 1)
    g = _r(gen, *out.shape)
    names = list(p)
    want = torch.autograd.grad(out, [x] + [p[n] for n in names], g)
    with torch.no_grad():
        kept = {}
        mine = B.mbconv_train_forward(x.detach(), p, k, s, same_pad(k, s)[0], e, residual, keep, kept=kept)
        _close(mine, out.detach(), 'forward')
        if residual:
            assert torch.equal(mine[1], x.detach()[1])             # the dropped image's branch contributes nothing
        grads, gx = B.mbconv_train_backward(g, p, kept, k, s, same_pad(k, s)[0], e, residual, keep)
    _close(gx, want[0], 'gx')
    assert sorted(grads) == sorted(names)
    for n, wv in zip(names, want[1:]):
        _close(grads[n], wv, n)


# ------------------------------------------------------------------------------------------------------- the interface
def test_train_is_the_fourth_value_and_false_is_still_refused(tmp_path):
    from vfloodnet_amd import train_image_seg as T
    from vfloodnet_amd.linknet import LinknetB4
    from vfloodnet_amd.linknet_train import ENCODER_MISSING, FullTrainer, ModelTrainer, train_mode
    assert T.TRAIN == 'train' and "freeze_encoder='train'" in ENCODER_MISSING
    assert T._check_mode('train') == 'train'
    with pytest.raises(RuntimeError, match='GPU only'):          # passes the mode check and stops at the device: no CPU fallback
        T.TrainEpoch(None, 'cpu', freeze_encoder='train')
    for bad in (False, None, 0):
        with pytest.raises(NotImplementedError, match="freeze_encoder='train'"):
            T.TrainEpoch(None, 'cuda', freeze_encoder=bad)
    with pytest.raises(ValueError, match="'train'"):
        T.TrainEpoch(None, 'cuda', freeze_encoder='training')
    assert issubclass(FullTrainer, ModelTrainer)
    model = LinknetB4()
    model.eval()
    assert train_mode(model) is model and model.training and model.encoder.training and model.decoder.training
    assert all(p.requires_grad for p in model.parameters())
    with pytest.raises(RuntimeError, match='HIP device only'):   # the mode's optimizer: built over the model in train mode, on the GPU
        T.new_optimizer(model.eval(), 'train', 1e-3)
    assert model.training and model.encoder.training
    from test_encoder_train_ref_host import _host_adam          # (linknet_train.Adam's bookkeeping with its buffers on the CPU)
    from vfloodnet_amd.linknet_train import UNUSED, freeze_encoder, freeze_encoder_statistics
    opt = _host_adam(model, UNUSED)
    assert opt.n_group == 468 and len(opt.names) == 465
    # a checkpoint of decoder-only training is refused by a message that names both whole-model modes
    small = _host_adam(freeze_encoder(LinknetB4()), ())
    with pytest.raises(ValueError) as e:
        T.load_optimizer_state(opt, small.state_dict(), 'train')
    assert '--train-encoder' in str(e.value) and '--freeze-encoder-statistics' in str(e.value) and '--freeze-encoder)' in str(e.value)
    # 'statistics' and 'train' resume each other: the same 468 numbered parameters and state for 465
    stats = _host_adam(freeze_encoder_statistics(LinknetB4()), UNUSED)
    stats.step_count = 2
    T.load_optimizer_state(opt, stats.state_dict(), 'train')
    assert opt.step_count == 2
    T.load_optimizer_state(stats, opt.state_dict(), 'statistics')


def test_command_line_flag():
    from vfloodnet_amd import train_image_seg as T
    base = ['--dataset-path', 'x', '--model-path', 'y']
    a = T.get_args(base + ['--train-encoder', '--seed', '5'])
    assert a.train_encoder and not a.freeze_encoder and not a.freeze_encoder_statistics and a.seed == 5
    for other in ('--freeze-encoder', '--freeze-encoder-statistics'):
        with pytest.raises(SystemExit):
            T.get_args(base + ['--train-encoder', other])
    with pytest.raises(NotImplementedError, match='--train-encoder'):
        T.main(base)
    with pytest.raises(ValueError, match='CUDA is required|--gpu'):
        T.main(base + ['--train-encoder', '--gpu', '-1'])


def test_bad_arguments_are_refused_before_any_launch():
    """The entry points check their arguments on the host: with pointers that are never dereferenced every bad call comes back
    as VFN_ERR_ARG (1) without a device."""
    from vfloodnet_amd import _lib
    L = _lib.lib()
    x, v, k, o, p = (ctypes.c_void_p(4096 * (i + 1)) for i in range(5))
    bad = B.refusals(L, x, v, k, o, p, None)
    assert len(bad) > 55 and all(st == 1 for _, _, st in bad), [b for b in bad if b[2] != 1]


# ---------------------------------------------------------------------------------------------------- the conditioning
@pytest.mark.parametrize('batch', B.BATCHES)
def test_float32_reference_stays_within_the_cap_under_the_tests_table(batch):
    """The error rule of the device tests is FACTOR x the float32 reference's distance from float64, in units of the kind's
    scale; an ill-conditioned input would loosen it, so the cap is held here for the table the device tests pass.  Measured:
    (2, 64, 64) 5.2e-5 (gradients), 1.8e-5 (taps); (3, 64, 96) 1.2e-5, 9.3e-6."""
    P = B.reference_pass(batch)
    (feats, ref, stats), (feats32, r32, stats32) = P['ref'], P['r32']
    assert len(ref) == 413 and len(stats) == 190
    d = B.distances(r32, ref, B.kind_scales(ref))
    worst = max(d, key=d.get)
    taps = [(a.double() - b).abs().max().item() / b.abs().max().item() for a, b in zip(feats32, feats)]
    sd = B.distances(stats32, stats, {n: v.abs().max().item() for n, v in stats.items()})
    print(f'{batch}: float32 from float64: gradients {d[worst]:.2e} at {worst}, taps {max(taps):.2e}, running statistics {max(sd.values()):.2e}')
    assert d[worst] < B.CAP and max(taps) < B.CAP and max(sd.values()) < B.CAP
    # the kinds' scales are what the issue expects: large, from the batch rstd at small M
    assert min(B.kind_scales(ref).values()) > 1.0
