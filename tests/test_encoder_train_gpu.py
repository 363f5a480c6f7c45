"""Training the whole LinkNet with the encoder's BatchNorm statistics frozen (``linknet_train.ModelTrainer``,
``train_image_seg`` with ``freeze_encoder='statistics'``) on the synthetic checkpoint of ``tools/synth_linknet.py``.

The encoder is held on its own against float64 autograd through ``oracle/linknet_ref.encoder`` (a smooth chain: swish and
sigmoid only), the decoder's feature gradients against float64 autograd through the decoder fed with the device's own taps;
the whole model is NOT differentiated in one piece against the device: the decoder's ReLUs sit 1e-6 .. 1e-7 of a layer's rms
from zero on these inputs and float32 and float64 disagree about one of them for every second seed.

The error rule is tests/test_image_train_gpu.py's: the reference run in float32 on the CPU lies ``e32 / |ref|max`` from the
float64 run; the device may be 8 x the largest such ratio over the batches away, in units of the tensor's own ``|ref|max``."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import encoder_train_ref as R
import linknet_train_ref as R0
from test_image_train_gpu import make_batch

pytestmark = pytest.mark.gpu

FACTOR = 8.0
ENCODER_BATCHES = [(2, 64, 64), (3, 64, 96), (1, 32, 32)]
BATCHES = [(2, 64, 64), (3, 64, 96)]
LR = 1e-3
TAPS = R.TAP_CHANNELS


@pytest.fixture(scope='module')
def state():
    from tools import synth_linknet
    return synth_linknet.make_state_dict()


def fresh(state, gpu, lr=LR, cls=None):
    from vfloodnet_amd.linknet import LinknetB4
    from vfloodnet_amd import linknet_train
    model = LinknetB4.from_checkpoint(state, gpu)
    return model, (cls or linknet_train.ModelTrainer)(model, init_lr=lr)


def nchw(t, c):
    """A tap (or its gradient) as the device holds it -> [N, c, h, w] float64 on the CPU; the padding must be zero."""
    assert not t[..., c:].any()
    return t[..., :c].permute(0, 3, 1, 2).double().cpu()


def hold(what, runs, batches):
    """runs: per batch a list of (name, float32 distance, device distance).  A tensor's bound is 8 x its largest float32
    distance over the batches."""
    bound = {}
    for rows in runs:
        for name, e32, _ in rows:
            bound[name] = max(bound.get(name, 0.0), e32)
    bad = [(b, name, f'error {e:.3e}', f'bound {FACTOR * bound[name]:.3e}') for b, rows in zip(batches, runs) for name, _, e in rows
           if not e <= FACTOR * bound[name]]
    worst = max(((e / (FACTOR * bound[name]) if bound[name] > 0 else (0.0 if e == 0 else float('inf')), name) for rows in runs for name, _, e in rows))
    print(f'{what}: {sum(len(r) for r in runs)} tensors; largest float32 distance {max(bound.values()):.3e}; worst tensor {worst[1]} at '
          f'{worst[0]:.3f} of its bound')
    assert not bad, (what, len(bad), bad[:6])


# ------------------------------------------------------------------------------------------------ 1. the encoder alone
def test_encoder_backward_equals_float64_autograd(gpu, state):
    """``encoder_forward`` then ``encoder_backward`` from given tap gradients (seeded normal / sqrt(C)) against float64
    ``torch.autograd.grad`` through ``oracle/linknet_ref.encoder``, all 413 tensors, and the taps against the oracle's features.
    Measured on the CPU: the float32 reference stays within 3.5e-6 / 4.9e-6 / 7.1e-6 of float64 on every tensor of the three
    batches and the smallest |g|max is 1e-3, so the bound is below 6e-5; an ill-conditioned input (float32 beyond 1e-4) fails
    loudly instead of loosening it."""
    runs, tap_runs = [], []
    names = R.encoder_names(state)
    assert len(names) == 413
    for N, H, W in ENCODER_BATCHES:
        model, trainer = fresh(state, gpu)
        x = make_batch(N, H, W)[0]
        gen = torch.Generator().manual_seed(1000 + H + W)
        gt = [torch.randn(N, c, H >> (i + 1), W >> (i + 1), generator=gen) / c ** 0.5 for i, c in enumerate(TAPS)]
        taps = trainer.encoder_forward(x.to(gpu))
        gdev = []
        for t, g in zip(taps, gt):
            d = torch.zeros_like(t)
            d[..., :g.shape[1]] = g.permute(0, 2, 3, 1).to(gpu)
            gdev.append(d)
        keep = [g.clone() for g in gdev]
        grads = trainer.encoder_backward(gdev)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(gdev, keep))                 # the caller's gradients are not written to
        feats, ref = R.encoder_reference(state, x, gt)
        feats32, r32 = R.encoder_reference(state, x, gt, dtype=torch.float32)
        assert sorted(grads) == sorted(names)
        rows = []
        for n in names:
            got, want = grads[n].detach().cpu().double(), ref[n]
            assert got.shape == want.shape, n
            scale = want.abs().max().item()
            rows.append((n, (r32[n].double() - want).abs().max().item() / scale, (got - want).abs().max().item() / scale))
        assert max(r[1] for r in rows) < 1e-4, ('ill-conditioned input', (N, H, W), max(rows, key=lambda r: r[1]))
        runs.append(rows)
        tap_runs.append([(f'tap {i}', (f32.double() - f).abs().max().item() / f.abs().max().item(),
                          (nchw(t, c) - f).abs().max().item() / f.abs().max().item())
                         for i, (t, c, f, f32) in enumerate(zip(taps, TAPS, feats, feats32))])
    hold('encoder taps', tap_runs, ENCODER_BATCHES)
    hold('encoder backward', runs, ENCODER_BATCHES)


# --------------------------------------------------------------------------- 2. / 3. the decoder's hand-over, the composition
@functools.lru_cache(maxsize=None)
def _pass(batch):
    """One ``forward_backward`` of a fresh model on a batch, beside the float64 / float32 decoder references fed with the device's
    own taps; computed once for the tests below."""
    from tools import synth_linknet
    state = synth_linknet.make_state_dict()
    gpu = torch.device('cuda', 0)
    N, H, W = batch
    model, trainer = fresh(state, gpu)
    x, y = (t.to(gpu) for t in make_batch(N, H, W))
    taps = [t.clone() for t in trainer.encoder_forward(x)]
    trainer.esaved = None
    torch.cuda.synchronize()
    feats = [nchw(t, c) for t, c in zip(taps, TAPS)][::-1]
    ref = R.decoder_reference(model, feats, y.cpu())           # (before the device's pass moves the running statistics)
    r32 = R.decoder_reference(model, feats, y.cpu(), dtype=torch.float32)
    fg = []
    loss, grads = trainer.forward_backward(x, y, feat_grads=fg)
    grads = {k: v.detach().clone() for k, v in grads.items()}
    torch.cuda.synchronize()
    return dict(model=model, trainer=trainer, x=x, y=y, loss=loss, grads=grads, fg=fg, ref=ref, r32=r32)


def test_feature_gradients_equal_float64_autograd(gpu):
    """The gradients of the five taps the decoder's backward hands over, against float64 autograd through a deep copy of the
    decoder and head in train mode with the device's own taps as leaves."""
    runs = []
    for b in BATCHES:
        P = _pass(b)
        want, w32 = P['ref'][4][::-1], P['r32'][4][::-1]                          # shallowest first, as the taps
        assert len(P['fg']) == 5
        runs.append([(f'tap {i} grad', (w32[i].double() - want[i]).abs().max().item() / want[i].abs().max().item(),
                      (nchw(P['fg'][i], TAPS[i]) - want[i]).abs().max().item() / want[i].abs().max().item()) for i in range(5)])
    hold('feature gradients', runs, BATCHES)


def test_forward_backward_is_the_two_halves_around_the_decoder(gpu):
    """The 413 encoder gradients of ``forward_backward`` are ``encoder_backward`` of the tap gradients above, bit for bit; its
    52 decoder gradients, the loss and the 30 running statistics hold the decoder-only comparison."""
    runs = []
    for b in BATCHES:
        P = _pass(b)
        trainer, grads, ref, r32 = P['trainer'], P['grads'], P['ref'], P['r32']
        assert len(grads) == 465
        trainer.encoder_forward(P['x'])
        again = trainer.encoder_backward(P['fg'])
        torch.cuda.synchronize()
        assert len(again) == 413 and all(torch.equal(again[k], grads[k]) for k in again)
        rows = [('loss', abs(float(r32[0]) - float(ref[0])) / abs(float(ref[0])), abs(float(P['loss']) - float(ref[0])) / abs(float(ref[0])))]
        assert sorted(k for k in grads if not k.startswith('encoder.')) == sorted(ref[1]) and len(ref[1]) == 52
        for name, want in ref[1].items():
            got = grads[name].cpu().double()
            assert got.shape == want.shape, name
            scale = ref[3][name].max().item() if name in ref[3] else want.abs().max().item()
            rows.append((name + ' grad', (r32[1][name].double() - want).abs().max().item() / scale, (got - want).abs().max().item() / scale))
        sd = P['model'].state_dict()
        n = 0
        for name, want in ref[2].items():
            if name.endswith('num_batches_tracked'):
                assert int(sd[name]) == int(want), name
                continue
            n += 1
            scale = want.abs().max().item()
            rows.append((name, (r32[2][name].double() - want).abs().max().item() / scale, (sd[name].cpu().double() - want).abs().max().item() / scale))
        assert n == 30
        runs.append(rows)
    hold('decoder inside the whole step', runs, BATCHES)


# -------------------------------------------------------------------------------------------------------------- 4. the step
def test_step_moves_465_tensors_by_float64_adam(gpu, state):
    """After ``step`` all 465 tensors moved, the three unused ones and every encoder running statistic are bit-equal to before;
    the parameters hold against float64 Adam on the device's gradients under the bound of
    ``test_parameters_after_a_step_equal_float64_adam``: 2 * 2^-23 |p|max + 1e-5 lr.  The optimizer's state dict numbers all
    468 parameters, holds state for 465 and loads into ``torch.optim.Adam`` on a CPU copy, and back."""
    N, H, W = BATCHES[0]
    model, trainer = fresh(state, gpu)
    x, y = (t.to(gpu) for t in make_batch(N, H, W))
    everyone = [n for n, _ in model.named_parameters()]
    names = [n for n in everyone if n not in R.UNUSED]
    assert len(everyone) == 468 and len(names) == 465 and trainer.optimizer.names == names and all(p.requires_grad for p in model.parameters())
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    _, grads = trainer.forward_backward(x, y)
    grads = {k: v.detach().clone() for k, v in grads.items()}
    trainer.step(x, y)
    torch.cuda.synchronize()
    after = model.state_dict()
    assert all(not torch.equal(after[n], before[n]) for n in names), [n for n in names if torch.equal(after[n], before[n])][:5]
    assert all(torch.equal(after[n], before[n]) for n in R.UNUSED)
    frozen = [k for k in before if k.startswith('encoder.') and k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))]
    assert len(frozen) == 3 * 96 and all(torch.equal(after[k], before[k]) for k in frozen)
    worst = 0.0
    for n in names:
        want, _, _ = R0.adam_step(before[n].cpu(), grads[n].cpu(), torch.zeros_like(before[n]).cpu(), torch.zeros_like(before[n]).cpu(), 1, LR)
        err = (after[n].detach().cpu().double() - want).abs().max().item()
        bound = 2 * 2.0 ** -23 * before[n].abs().max().item() + 1e-5 * LR
        worst = max(worst, err / bound)
        assert err <= bound, (n, err, bound)
    print(f'adam over 465 tensors: worst at {worst:.3f} of its bound')
    sd = trainer.optimizer.state_dict()
    cpu = copy.deepcopy(model).to('cpu')
    topt = torch.optim.Adam([dict(params=cpu.parameters(), lr=LR)])
    assert sd['param_groups'][0] == topt.state_dict()['param_groups'][0] and sd['param_groups'][0]['params'] == list(range(468))
    assert sorted(sd['state']) == [everyone.index(n) for n in names]
    topt.load_state_dict(sd)
    back = topt.state_dict()
    assert len(back['state']) == 465 and float(back['state'][0]['step']) == 1.0
    trainer.optimizer.load_state_dict(back)
    again = trainer.optimizer.state_dict()
    assert all(torch.equal(again['state'][i]['exp_avg'], sd['state'][i]['exp_avg']) for i in sd['state'])


def test_predict_after_training_equals_the_oracle(gpu, state):
    """``predict_batch`` / ``predict`` after three steps: the oracle's eval forward on the new state dict, within
    tests/test_linknet.py's bound (logits 2e-3 absolute, probabilities 5e-4); the packed inference filters followed."""
    from oracle import linknet_ref as O
    N, H, W = BATCHES[1]
    model, trainer = fresh(state, gpu)
    x, y = (t.to(gpu) for t in make_batch(N, H, W))
    stale = model.predict_batch(x, logits=True).clone()
    for _ in range(3):
        trainer.step(x, y)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        z_ref = O.logits({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, x.cpu().double())
    z = model.predict_batch(x, logits=True).cpu().double()
    p = model.predict(x).cpu().double()
    err, perr = (z - z_ref).abs().max().item(), (p - torch.sigmoid(z_ref)).abs().max().item()
    print(f'predict after 3 steps: max |dlogit| {err:.2e}, max |dprob| {perr:.2e}; the logits moved by {(z - stale.cpu().double()).abs().max().item():.2e}')
    assert err < 2e-3 and perr < 5e-4
    assert (z - stale.cpu().double()).abs().max().item() > 10 * 2e-3
    assert not torch.equal(sd['encoder._blocks.5._depthwise_conv.weight'], state['encoder._blocks.5._depthwise_conv.weight'])


def test_twenty_steps_lower_the_dice_loss_further_than_the_decoder_alone(gpu, state):
    """One fixed batch (64 x 64, batch 2, seed 40), lr 1e-3, twenty steps from the same start: training the encoder as well
    lowers the Dice loss, and by more than the decoder-only trainer does.  The assertion is the ordering."""
    from vfloodnet_amd.linknet_train import DecoderTrainer
    N, H, W = BATCHES[0]
    out = {}
    for cls in (None, DecoderTrainer):
        model, trainer = fresh(state, gpu, cls=cls)
        x, y = (t.to(gpu) for t in make_batch(N, H, W))
        out[cls] = torch.stack([trainer.step(x, y)['dice_loss'] for _ in range(21)]).cpu().tolist()
    full, dec = out[None], out[DecoderTrainer]
    print(f'dice loss, 20 steps: whole model {full[0]:.4f} -> {full[20]:.4f}; decoder and head only {dec[0]:.4f} -> {dec[20]:.4f}')
    assert abs(full[0] - dec[0]) < 1e-6                          # the same start
    assert full[20] < full[0] and full[0] - full[20] > dec[0] - dec[20]


# --------------------------------------------------------------------------------------------------------------- 5. the CLI
def test_command_line_trains_the_encoder_for_one_epoch(gpu, state, tmp_path, capsys):
    """The synthetic set of tests/test_image_train_gpu.py's command-line test, one epoch with --freeze-encoder-statistics: the
    best model it writes loads into ``LinknetB4.from_checkpoint`` and its encoder differs from the start; resuming it with
    --freeze-encoder is refused by a message that names the two modes."""
    from PIL import Image
    from tools import synth
    from vfloodnet_amd import train_image_seg
    from vfloodnet_amd.linknet import LinknetB4
    root = tmp_path / 'water'
    os.makedirs(root / 'JPEGImages' / 'a')
    os.makedirs(root / 'Annotations' / 'a')
    (root / 'train_imgs.txt').write_text('a\n')
    for k in range(4):
        f0, m = synth.frame0(60 + k, 72 + 8 * (k % 2), 96)
        Image.fromarray((f0.permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)).save(root / 'JPEGImages' / 'a' / f'{k}.jpg', quality=92)
        pm = Image.fromarray(m.numpy().astype(np.uint8), 'P')
        pm.putpalette([0, 0, 0, 0, 0, 128] + [100] * (254 * 3))
        pm.save(root / 'Annotations' / 'a' / f'{k}.png')
    start = str(tmp_path / 'start.pth')
    torch.save(state, start)
    out = tmp_path / 'out'
    common = ['--dataset-path', str(root), '--encoder', 'efficientnet-b4', '--input-shape', '64', '--batch-size', '2', '--init-lr', '1e-3',
              '--epochs', '1', '--seed', '3', '--num-workers', '0']
    history = train_image_seg.main(common + ['--out-path', str(out), '--model-path', start, '--freeze-encoder-statistics'])
    printed = capsys.readouterr().out
    assert len(history) == 1 and 'train: dice_loss - ' in printed and 'Done.' in printed
    ck = os.listdir(out / 'checkpoints')
    assert len(ck) == 1
    obj = torch.load(out / 'checkpoints' / ck[0], map_location='cpu', weights_only=True)
    assert sorted(obj) == ['epoch', 'loss', 'optimizer', 'weights'] and len(obj['optimizer']['state']) == 465
    assert obj['optimizer']['param_groups'][0]['params'] == list(range(468)) and float(obj['optimizer']['state'][0]['step']) == 2.0
    moved = [k for k in R.encoder_names(state) if not torch.equal(obj['weights'][k], state[k])]
    assert len(moved) == 413
    assert all(torch.equal(obj['weights'][k], state[k]) for k in R.UNUSED)
    best = os.listdir(out / 'model')                               # a half-water scene scores above 0: the epoch's model is the best
    assert len(best) == 1 and history[0][3]
    model = LinknetB4.from_checkpoint(str(out / 'model' / best[0]), gpu)
    sd = model.state_dict()
    assert all(torch.equal(sd[k].cpu(), obj['weights'][k]) for k in obj['weights'])
    assert not torch.equal(sd['encoder._conv_stem.weight'].cpu(), state['encoder._conv_stem.weight'])
    with pytest.raises(ValueError, match='freeze-encoder-statistics'):
        train_image_seg.main(common + ['--out-path', str(tmp_path / 'out2'), '--model-path', str(out / 'checkpoints' / ck[0]), '--freeze-encoder'])
