"""``tests/linknet_train_ref.py`` against ``torch.autograd`` (CPU, float64): the five kernel formulas of
include/vfn_image_train.h, the running-statistics rule against ``nn.BatchNorm2d``, one decoder block chained from the formulas
and the convolution identities ``vfloodnet_amd/linknet_train.py`` relies on, the optimizer's state-dict layout, and
``train_model``'s files, ``score > max_score`` rule and half-way learning-rate drop with stub epochs."""
import os

import pytest
import torch
import torch.nn.functional as F

import linknet_train_ref as R

D = torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize('N,C,h,w', [(1, 4, 1, 2), (2, 8, 3, 5), (3, 12, 4, 4)])
def test_batchnorm_formulas_equal_autograd(N, C, h, w):
    g_ = _gen(N * 100 + C)
    x = torch.randn(N, C, h, w, dtype=D, generator=g_, requires_grad=True)
    gamma = (1 + 0.3 * torch.randn(C, dtype=D, generator=g_)).requires_grad_(True)
    beta = (0.2 * torch.randn(C, dtype=D, generator=g_)).requires_grad_(True)
    gy = torch.randn(N, C, h, w, dtype=D, generator=g_)
    bn = torch.nn.BatchNorm2d(C, eps=R.BN_EPS, momentum=R.BN_MOMENTUM).double().train()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(C, dtype=D, generator=g_))
        bn.running_var.copy_(0.5 + torch.rand(C, dtype=D, generator=g_))
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    y_mod = bn(x.detach())
    y = F.relu(F.batch_norm(x, None, None, gamma, beta, True, R.BN_MOMENTUM, R.BN_EPS))
    (y * gy).sum().backward()
    xr, gr = R._rows(x.detach()), R._rows(gy)
    s = R.bn_stats(xr, gamma.detach(), beta.detach(), rm0, rv0)
    tol = dict(rtol=0, atol=1e-12)
    assert torch.allclose(R._image(R.bn_apply(xr, s['scale'], s['shift']), N, h, w), y.detach(), **tol)
    assert torch.allclose(R._image(R.bn_apply(xr, s['scale'], s['shift'], relu=False), N, h, w), y_mod.detach(), **tol)
    assert torch.allclose(s['running_mean'], bn.running_mean, **tol) and torch.allclose(s['running_var'], bn.running_var, **tol)
    assert int(bn.num_batches_tracked) == 1
    dg, db, _, _ = R.bn_bwd_reduce(gr, xr, s['scale'], s['shift'], s['mean'], s['rstd'])
    assert torch.allclose(dg, gamma.grad, **tol) and torch.allclose(db, beta.grad, **tol)
    gx = R.bn_bwd_apply(gr, xr, s['scale'], s['shift'], s['mean'], s['rstd'], dg, db)
    assert torch.allclose(R._image(gx, N, h, w), x.grad, **tol)


def test_one_value_per_channel_is_refused_by_torch():
    """What the product's ValueError restates."""
    with pytest.raises(ValueError, match='more than 1 value per channel'):
        F.batch_norm(torch.zeros(1, 4, 1, 1), None, None, torch.ones(4), torch.zeros(4), True, 0.1, 1e-5)


def test_head_formula_equals_autograd():
    g_ = _gen(7)
    M = 150
    x = torch.randn(M, 32, dtype=D, generator=g_, requires_grad=True)
    w = (0.3 * torch.randn(32, dtype=D, generator=g_)).requires_grad_(True)
    b = torch.tensor(0.1, dtype=D, requires_grad=True)
    gt = (torch.rand(M, dtype=D, generator=g_) > 0.6).to(D)
    pr = torch.sigmoid(x @ w + b)
    loss = R.dice_loss(pr, gt)
    loss.backward()
    gx, gw, gb, _ = R.head_bwd(x.detach(), w.detach(), pr.detach(), gt)
    tol = dict(rtol=0, atol=1e-14)
    assert torch.allclose(gx, x.grad, **tol) and torch.allclose(gw, w.grad, **tol) and torch.allclose(gb, b.grad, **tol)
    s0, s1, s2 = R.dice_sums(pr.detach(), gt)
    assert float(loss.detach()) == float(1 - (2 * s0 + 1) / (s1 + s2 + 1))
    assert float(R.dice_loss(torch.zeros(5, dtype=D), torch.zeros(5, dtype=D))) == 0.0


@pytest.mark.parametrize('N,cin,mid,cout,h,w', [(2, 8, 2, 6, 2, 3), (1, 12, 3, 4, 1, 2)])
def test_block_chain_equals_autograd(N, cin, mid, cout, h, w):
    """Conv -> BN -> ReLU -> ConvTranspose2d(4, 2, 1) -> BN -> ReLU -> conv -> BN -> ReLU in training mode: the formulas chained
    with the transposed convolution as the 4x4 convolution of the zero-inserted input, its weight gradient mapped back to
    Wt[i][o][kh][kw], and its data gradient as the 4x4 / stride-2 / pad-1 convolution with Wt's own layout."""
    g_ = _gen(cin * 10 + mid)
    r = lambda *s: torch.randn(*s, dtype=D, generator=g_)
    P = dict(w_a=r(mid, cin, 1, 1), g_a=1 + 0.2 * r(mid), b_a=0.2 * r(mid), wt=0.5 * r(mid, mid, 4, 4), bias=0.3 * r(mid),
             g_t=1 + 0.2 * r(mid), b_t=0.2 * r(mid), w_c=r(cout, mid, 1, 1), g_c=1 + 0.2 * r(cout), b_c=0.2 * r(cout))
    x, g_out = r(N, cin, h, w), r(N, cout, 2 * h, 2 * w)
    out, grads, gx = R.block_forward_backward(x, P, g_out)
    Q = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    xa = x.clone().requires_grad_(True)
    bn = lambda t, g, b: F.relu(F.batch_norm(t, None, None, g, b, True, 0.1, R.BN_EPS))
    a = bn(F.conv2d(xa, Q['w_a']), Q['g_a'], Q['b_a'])
    assert torch.allclose(R.transposed_as_conv(a.detach(), P['wt'], P['bias']),
                          F.conv_transpose2d(a.detach(), P['wt'], P['bias'], stride=2, padding=1), rtol=0, atol=1e-12)
    t = bn(F.conv_transpose2d(a, Q['wt'], Q['bias'], stride=2, padding=1), Q['g_t'], Q['b_t'])
    ref = bn(F.conv2d(t, Q['w_c']), Q['g_c'], Q['b_c'])
    (ref * g_out).sum().backward()
    assert torch.allclose(out, ref.detach(), rtol=0, atol=1e-11)
    for k in P:
        scale = max(1.0, float(Q[k].grad.abs().max()))
        assert float((grads[k] - Q[k].grad).abs().max()) <= 1e-10 * scale, k
    assert float((gx - xa.grad).abs().max()) <= 1e-10 * max(1.0, float(xa.grad.abs().max()))
    assert float(grads['bias'].abs().max()) <= 1e-10 * float(R._rows(g_out).abs().sum())      # BatchNorm removes the mean: ~0


def test_decoder_reference_covers_the_52_trained_tensors():
    from vfloodnet_amd.linknet import LinknetB4, DEC_CHANNELS
    torch.manual_seed(3)
    model = LinknetB4()
    feats = [torch.randn(2, c, 2 * 2 ** j, 3 * 2 ** j, dtype=D) for j, c in enumerate(DEC_CHANNELS[:5])]
    y = (torch.rand(2, 1, 64, 96) > 0.5).to(D)
    loss, grads, stats, pr, abs_sums = R.decoder_reference(model, feats, y)
    assert sorted(abs_sums) == [f'decoder.blocks.{j}.block.1.0.bias' for j in range(5)]
    for k, v in abs_sums.items():
        assert float((grads[k].abs() / v).max()) < 1e-12                  # BatchNorm removes the mean: zero up to rounding
    trained = [n for n, _ in model.named_parameters() if n.startswith(R.TRAINED_PREFIXES)]
    assert len(trained) == 52 and sorted(grads) == sorted(trained) and pr.shape == (2, 1, 64, 96) and 0 < float(loss) < 1
    assert len([k for k in stats if k.endswith(('running_mean', 'running_var'))]) == 30
    assert all(int(v) == 1 for k, v in stats.items() if k.endswith('num_batches_tracked'))
    assert all(int(b.num_batches_tracked) == 0 for b in model.decoder.modules() if isinstance(b, torch.nn.BatchNorm2d))   # a copy was trained
    assert torch.equal(model.decoder.blocks[0].block[0][1].running_mean, torch.zeros(112))


def test_adam_restatement_equals_torch():
    g_ = _gen(5)
    p = torch.randn(40, dtype=D, generator=g_)
    q = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([dict(params=[q], lr=1e-3)])
    m, v = torch.zeros(40, dtype=D), torch.zeros(40, dtype=D)
    for step in (1, 2, 3):
        g = torch.randn(40, dtype=D, generator=g_)
        q.grad = g.clone()
        opt.step()
        p, m, v = R.adam_step(p, g, m, v, step, 1e-3)
        assert torch.allclose(p, q.detach(), rtol=0, atol=1e-14)


# ------------------------------------------------------------------------------------------------------------ train_model
class _StubOptimizer:
    def __init__(self, lr):
        self.lr = lr

    def state_dict(self):
        return {'state': {}, 'param_groups': [{'lr': self.lr, 'params': []}]}


class _StubEpoch:
    def __init__(self, scores, optimizer=None):
        self.scores, self.calls, self.optimizer, self.lrs = list(scores), 0, optimizer, []

    def run(self, loader):
        if self.optimizer is not None:
            self.lrs.append(self.optimizer.lr)
        score = self.scores[self.calls]
        self.calls += 1
        return {'dice_loss': 1.0 - score, 'iou_score': score}


def test_train_model_files_best_rule_and_learning_rate_drop(tmp_path):
    from vfloodnet_amd import train_image_seg as T
    from vfloodnet_amd.linknet import LinknetB4
    model = LinknetB4()
    scores = [0.0, 0.25, 0.25, 0.5, 0.4]                          # zero selects nothing, a tie keeps the earlier one
    opt = _StubOptimizer(1e-4)
    train, valid = _StubEpoch([0.1] * 5, opt), _StubEpoch(scores)
    history = T.train_model(model, 1e-4, 5, str(tmp_path), None, None, 'efficientnet-b4', optimizer=opt, train_epoch=train, valid_epoch=valid)
    assert [h[3] for h in history] == [False, True, False, True, False]
    assert train.lrs == [1e-4, 1e-4, 1e-4, 1e-5, 1e-5] and int(5 / 2) == 2      # the drop follows epoch 2
    ck = sorted(os.listdir(tmp_path / 'checkpoints'))
    assert ck == ['epoch_%03d_score%s.pth' % (e, str(float(s))) for e, s in enumerate(scores)]
    assert sorted(os.listdir(tmp_path / 'model')) == ['linknet_efficientnet-b4_epoch_001_score0.25.pth', 'linknet_efficientnet-b4_epoch_003_score0.5.pth']
    obj = torch.load(tmp_path / 'checkpoints' / ck[3], map_location='cpu', weights_only=True)
    assert sorted(obj) == ['epoch', 'loss', 'optimizer', 'weights'] and obj['epoch'] == 3 and obj['loss'] == {}
    assert obj['optimizer']['param_groups'][0]['lr'] == 1e-5                    # (written after the drop that follows epoch 2)
    assert list(obj['weights']) == list(model.state_dict())
    best = torch.load(tmp_path / 'model' / 'linknet_efficientnet-b4_epoch_003_score0.5.pth', map_location='cpu', weights_only=True)
    LinknetB4.from_checkpoint(best, 'cpu')                                       # a state dict the product loads
    assert all(torch.equal(best[k], v) for k, v in model.state_dict().items())


def test_training_the_encoder_is_refused_by_name():
    from vfloodnet_amd import train_image_seg as T
    for call in (lambda: T.TrainEpoch(None, 'cuda', freeze_encoder=False),
                 lambda: T.train_model(None, 1e-4, 1, '.', None, None, freeze_encoder=False)):
        with pytest.raises(NotImplementedError) as e:
            call()
        for word in ('BatchNorm', 'drop-connect', 'depthwise', 'squeeze-excite'):
            assert word in str(e.value)
    with pytest.raises(ValueError, match='efficientnet-b4'):
        T.main(['--dataset-path', 'x', '--model-path', 'y', '--encoder', 'resnet34', '--freeze-encoder'])
    with pytest.raises(NotImplementedError):
        T.main(['--dataset-path', 'x', '--model-path', 'y'])
