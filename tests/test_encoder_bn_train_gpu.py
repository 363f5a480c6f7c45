"""Training the whole LinkNet with the encoder in train mode (``linknet_train.FullTrainer``, ``train_image_seg`` with
``freeze_encoder='train'``: batch-statistics BatchNorm and drop-connect in the encoder) on the synthetic checkpoint of
``tools/synth_linknet.py``, under the drop-connect table of ``encoder_bn_train_ref.tests_keep`` (three dropped images).

The encoder is held on its own against float64 autograd through ``encoder_bn_train_ref.encoder_train``; the decoder's feature
gradients against float64 autograd through the decoder fed with the device's own taps, as tests/test_encoder_train_gpu.py does.

The error rule: the reference run in float32 on the CPU lies ``e32`` from the float64 run; the device may be 8 x the largest such
distance over the batches away.  For the 413 gradients distances are in units of the largest ``|ref|max`` over the tensors of
the same kind (the same last two name components): in train mode a bias whose only consumers are convolution -> batch-statistics
BatchNorm has a gradient that is zero up to rounding, and its own ``|ref|max`` measures nothing.  The float32 reference stays
below 1e-4 (tests/test_encoder_bn_train_ref_host.py holds that for the table used here)."""
import os

import numpy as np
import pytest
import torch

import encoder_bn_train_ref as B
import encoder_train_ref as R
import linknet_train_ref as R0
from test_image_train_gpu import make_batch
from test_encoder_train_gpu import hold, nchw

pytestmark = pytest.mark.gpu

BATCHES = B.BATCHES
LR = 1e-3
HANDOVER_SEED = 69
TAPS = R.TAP_CHANNELS


@pytest.fixture(scope='module')
def state():
    from tools import synth_linknet
    return synth_linknet.make_state_dict()


def fresh(state, gpu, lr=LR, seed=0):
    from vfloodnet_amd.linknet import LinknetB4
    from vfloodnet_amd.linknet_train import FullTrainer
    model = LinknetB4.from_checkpoint(state, gpu)
    return model, FullTrainer(model, init_lr=lr, seed=seed)


def to_device_taps(taps, gt, gpu):
    out = []
    for t, g in zip(taps, gt):
        d = torch.zeros_like(t)
        d[..., :g.shape[1]] = g.permute(0, 2, 3, 1).to(gpu)
        out.append(d)
    return out


# ------------------------------------------------------------------------------------------------ 1. the encoder alone
def test_encoder_in_train_mode_equals_float64_autograd(gpu, state):
    """``encoder_forward(x, keep)`` then ``encoder_backward`` from given tap gradients against float64 autograd through the
    encoder in train mode: the five taps, all 413 gradients, all 190 running statistics and the 95 counters; a dropped image's
    branch contributes nothing: the block's output is its input, bit for bit."""
    names, stats = R.encoder_names(state), B.stat_names(state)
    assert len(names) == 413 and len(stats) == 190
    rates = B.drop_connect_rates()
    runs, tap_runs, stat_runs = [], [], []
    for batch in BATCHES:
        N, H, W = batch
        P = B.reference_pass(batch)
        (feats, ref, sref), (feats32, r32, s32) = P['ref'], P['r32']
        model, trainer = fresh(state, gpu)
        assert model.training and model.encoder.training and all(p.requires_grad for p in model.parameters())
        taps = trainer.encoder_forward(P['x'].to(gpu), keep=P['keep'])
        blocks = trainer.esaved['blocks']
        for r, n in B.TESTS_DROPS:
            i = rates[r][0]
            assert torch.equal(blocks[i + 1]['x'][n], blocks[i]['x'][n]), (i, n)
            assert not torch.equal(blocks[i + 1]['x'][(n + 1) % N], blocks[i]['x'][(n + 1) % N])
        gdev = to_device_taps(taps, P['gt'], gpu)
        kept = [g.clone() for g in gdev]
        grads = trainer.encoder_backward(gdev)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(gdev, kept))                 # the caller's gradients are not written to
        assert sorted(grads) == sorted(names) and all(grads[n].shape == ref[n].shape for n in names)
        scales = B.kind_scales(ref)
        e32, e = B.distances(r32, ref, scales), B.distances(grads, ref, scales)
        assert max(e32.values()) < B.CAP, ('ill-conditioned input', batch, max(e32, key=e32.get))
        runs.append([(n, e32[n], e[n]) for n in names])
        tap_runs.append([(f'tap {i}', (f32.double() - f).abs().max().item() / f.abs().max().item(),
                          (nchw(t, c) - f).abs().max().item() / f.abs().max().item())
                         for i, (t, c, f, f32) in enumerate(zip(taps, TAPS, feats, feats32))])
        sd = model.state_dict()
        own = {n: sref[n].abs().max().item() for n in stats}
        e32, e = B.distances(s32, sref, own), B.distances({n: sd[n] for n in stats}, sref, own)
        stat_runs.append([(n, e32[n], e[n]) for n in stats])
        assert all(not torch.equal(sd[n].cpu(), state[n]) for n in stats)
        counters = [k for k in sd if k.startswith('encoder.') and k.endswith('num_batches_tracked')]
        assert len(counters) == 96
        assert all(int(sd[k]) == int(state[k]) + (0 if k == 'encoder._bn1.num_batches_tracked' else 1) for k in counters)
        assert all(torch.equal(sd[k].cpu(), state[k]) for k in ('encoder._bn1.running_mean', 'encoder._bn1.running_var'))
    hold('train-mode encoder taps', tap_runs, BATCHES)
    hold('train-mode encoder running statistics', stat_runs, BATCHES)
    hold('train-mode encoder backward', runs, BATCHES)


# --------------------------------------------------------------------------- 2. the decoder's hand-over, the composition
def test_feature_gradients_and_the_two_halves_around_the_decoder(gpu, state):
    """``forward_backward(x, y, keep=...)``: the gradients of the five taps the decoder hands over, against float64 autograd through
    a deep copy of the decoder and head in train mode with the device's own taps as leaves; its 413 encoder gradients are
    ``encoder_backward`` of those, bit for bit; 465 gradients in all.

    The decoder is not smooth: a ReLU input that float32 and float64 place on different sides of zero changes these gradients by
    1e-2 (tests/test_encoder_train_gpu.py says the same of its batches).  The batch is therefore the seed, of 40 .. 71, whose
    float64 decoder pass keeps its ReLU inputs furthest from zero on both shapes (smallest |input| / rms over the fifteen layers:
    2.5e-6 and 1.5e-6 for seed 69 on the CPU reference's taps; the median seed has 4e-7).  The float32 reference on the CPU may
    still flip one (it did on one of two hosts, landing 9e-3 from float64 while the device lay 6e-7 away): its distance counts
    into a bound only up to the cap of the rule, so a flip there cannot loosen the bound beyond 8 x 1e-4."""
    runs = []
    for batch in BATCHES:
        N, H, W = batch
        keep = B.tests_keep(N)
        model, trainer = fresh(state, gpu)
        x, y = (t.to(gpu) for t in make_batch(N, H, W, seed=HANDOVER_SEED))
        taps = [t.clone() for t in trainer.encoder_forward(x, keep=keep)]
        trainer.esaved = None
        torch.cuda.synchronize()
        feats = [nchw(t, c) for t, c in zip(taps, TAPS)][::-1]
        ref = R.decoder_reference(model, feats, y.cpu())           # (before the device's pass moves the decoder's running statistics)
        r32 = R.decoder_reference(model, feats, y.cpu(), dtype=torch.float32)
        fg = []
        loss, grads = trainer.forward_backward(x, y, feat_grads=fg, keep=keep)
        grads = {k: v.detach().clone() for k, v in grads.items()}
        torch.cuda.synchronize()
        assert len(fg) == 5 and len(grads) == 465
        want, w32 = ref[4][::-1], r32[4][::-1]                     # shallowest first, as the taps
        rows = [(f'tap {i} grad', (w32[i].double() - want[i]).abs().max().item() / want[i].abs().max().item(),
                 (nchw(fg[i], TAPS[i]) - want[i]).abs().max().item() / want[i].abs().max().item()) for i in range(5)]
        rows.append(('loss', abs(float(r32[0]) - float(ref[0])) / abs(float(ref[0])), abs(float(loss) - float(ref[0])) / abs(float(ref[0]))))
        print(batch, [f'{name}: float32 {e32:.2e} device {e:.2e}' for name, e32, e in rows])
        runs.append([(name, min(e32, B.CAP), e) for name, e32, e in rows])
        trainer.encoder_forward(x, keep=keep)
        again = trainer.encoder_backward(fg)
        torch.cuda.synchronize()
        assert len(again) == 413 and all(torch.equal(again[k], grads[k]) for k in again)
    hold('train-mode feature gradients', runs, BATCHES)


# -------------------------------------------------------------------------------------------------------------- 3. the step
def test_step_moves_the_parameters_by_float64_adam_and_the_statistics(gpu, state):
    """After ``step`` the 465 tensors hold against float64 Adam on the device's gradients under the bound of
    tests/test_encoder_train_gpu.py (2 * 2^-23 |p|max + 1e-5 lr); the three unused tensors are bit-equal to before; the 190
    encoder running statistics moved and the counters counted both passes.  The optimizer's state dict numbers all 468
    parameters and holds state for 465."""
    N, H, W = BATCHES[0]
    keep = B.tests_keep(N)
    model, trainer = fresh(state, gpu)
    x, y = (t.to(gpu) for t in make_batch(N, H, W))
    everyone = [n for n, _ in model.named_parameters()]
    names = [n for n in everyone if n not in R.UNUSED]
    assert len(everyone) == 468 and trainer.optimizer.names == names
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    _, grads = trainer.forward_backward(x, y, keep=keep)
    grads = {k: v.detach().clone() for k, v in grads.items()}
    mid = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert all(torch.equal(mid[n], before[n]) for n in everyone)                  # gradients alone move no parameter
    logs = trainer.step(x, y, keep=keep)
    torch.cuda.synchronize()
    after = model.state_dict()
    assert 0.0 < float(logs['dice_loss']) < 1.0
    assert all(torch.equal(after[n], before[n]) for n in R.UNUSED)
    moved = sum(not torch.equal(after[n], before[n]) for n in names)
    assert moved >= 400, moved                                     # (a gradient that is zero up to rounding may round to no move)
    worst = 0.0
    for n in names:
        want, _, _ = R0.adam_step(before[n].cpu(), grads[n].cpu(), torch.zeros_like(before[n]).cpu(), torch.zeros_like(before[n]).cpu(), 1, LR)
        err = (after[n].detach().cpu().double() - want).abs().max().item()
        bound = 2 * 2.0 ** -23 * before[n].abs().max().item() + 1e-5 * LR
        worst = max(worst, err / bound)
        assert err <= bound, (n, err, bound)
    print(f'adam over 465 tensors in train mode: {moved} moved, worst at {worst:.3f} of its bound')
    stats = B.stat_names(state)
    assert all(not torch.equal(after[k], mid[k]) and not torch.equal(mid[k], before[k]) for k in stats)
    assert all(int(after[k[:k.rindex('.')] + '.num_batches_tracked']) == int(before[k[:k.rindex('.')] + '.num_batches_tracked']) + 2 for k in stats)
    sd = trainer.optimizer.state_dict()
    assert sd['param_groups'][0]['params'] == list(range(468)) and sorted(sd['state']) == [everyone.index(n) for n in names]
    assert float(sd['state'][0]['step']) == 1.0


def test_small_batches(gpu, state):
    """(1, 32, 32): one value per channel at the deepest stage: ``ValueError`` before anything is launched or moved, from ``step``
    and from ``encoder_forward``.  (2, 32, 32): two values there; no numeric case (the float32 reference itself is O(1) from
    float64), the step finishes and everything stays finite."""
    model, trainer = fresh(state, gpu)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    x, y = (t.to(gpu) for t in make_batch(1, 32, 32))
    with pytest.raises(ValueError, match='more than 1 value per channel'):
        trainer.step(x, y)
    with pytest.raises(ValueError, match='more than 1 value per channel'):
        trainer.encoder_forward(x)
    torch.cuda.synchronize()
    after = model.state_dict()
    assert trainer.esaved is None and trainer.saved is None and all(torch.equal(after[k], before[k]) for k in before)
    assert trainer.optimizer.step_count == 0
    x, y = (t.to(gpu) for t in make_batch(2, 32, 32))
    logs = trainer.step(x, y)
    assert np.isfinite(float(logs['dice_loss'])) and all(bool(torch.isfinite(v).all()) for v in model.state_dict().values())
    with pytest.raises(ValueError, match='25 blocks and 2 images'):
        trainer.step(x, y, keep=B.tests_keep(3))


def test_twenty_steps_lower_the_dice_loss(gpu, state):
    """One fixed batch (64 x 64, batch 2), lr 1e-3, twenty steps with the drop-connect scales drawn from the trainer's generator
    (seed 0): the Dice loss ends below its start, and the same seed gives the same losses, bit for bit.  The assertion is the
    direction; DESIGN.md 8g records the end value beside the float64 reference's."""
    N, H, W = BATCHES[0]
    out = []
    for _ in range(2):
        model, trainer = fresh(state, gpu, seed=0)
        x, y = (t.to(gpu) for t in make_batch(N, H, W))
        out.append(torch.stack([trainer.step(x, y)['dice_loss'] for _ in range(21)]).cpu().tolist())
    print(f'dice loss in train mode, 20 steps: {out[0][0]:.4f} -> {out[0][20]:.4f}')
    assert out[0][20] < out[0][0]
    assert out[0] == out[1]


def test_predict_after_training_equals_the_oracle_on_the_moved_statistics(gpu, state):
    """``predict_batch`` / ``predict`` after three steps: the oracle's eval forward on the new state dict -- new parameters AND the
    encoder's moved running statistics -- within tests/test_linknet.py's bound (logits 2e-3 absolute, probabilities 5e-4)."""
    from oracle import linknet_ref as O
    N, H, W = BATCHES[1]
    model, trainer = fresh(state, gpu)
    x, y = (t.to(gpu) for t in make_batch(N, H, W))
    stale = model.predict_batch(x, logits=True).clone()
    for _ in range(3):
        trainer.step(x, y, keep=B.tests_keep(N))
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        z_ref = O.logits({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, x.cpu().double())
    z = model.predict_batch(x, logits=True).cpu().double()
    p = model.predict(x).cpu().double()
    err, perr = (z - z_ref).abs().max().item(), (p - torch.sigmoid(z_ref)).abs().max().item()
    print(f'predict after 3 train-mode steps: max |dlogit| {err:.2e}, max |dprob| {perr:.2e}; the logits moved by '
          f'{(z - stale.cpu().double()).abs().max().item():.2e}')
    assert err < 2e-3 and perr < 5e-4
    assert (z - stale.cpu().double()).abs().max().item() > 10 * 2e-3
    assert not torch.equal(sd['encoder._blocks.5._bn1.running_var'], state['encoder._blocks.5._bn1.running_var'])
    assert int(sd['encoder._blocks.5._bn1.num_batches_tracked']) == int(state['encoder._blocks.5._bn1.num_batches_tracked']) + 3


# --------------------------------------------------------------------------------------------------------------- 4. the CLI
def test_command_line_trains_one_epoch_and_resumes(gpu, state, tmp_path, capsys):
    """The synthetic set of tests/test_image_train_gpu.py's command-line test, one epoch with --train-encoder: the checkpoint
    numbers 468 parameters with state for 465, the encoder's parameters and running statistics moved; --resume continues it at
    epoch 1, and --freeze-encoder-statistics resumes it as well (the same parameters)."""
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
              '--seed', '3', '--num-workers', '0']
    history = train_image_seg.main(common + ['--epochs', '1', '--out-path', str(out), '--model-path', start, '--train-encoder'])
    printed = capsys.readouterr().out
    assert len(history) == 1 and 'train: dice_loss - ' in printed and 'Done.' in printed
    ck = os.listdir(out / 'checkpoints')
    assert len(ck) == 1
    obj = torch.load(out / 'checkpoints' / ck[0], map_location='cpu', weights_only=True)
    assert sorted(obj) == ['epoch', 'loss', 'optimizer', 'weights'] and len(obj['optimizer']['state']) == 465
    assert obj['optimizer']['param_groups'][0]['params'] == list(range(468)) and float(obj['optimizer']['state'][0]['step']) == 2.0
    assert sum(not torch.equal(obj['weights'][k], state[k]) for k in R.encoder_names(state)) >= 400
    assert all(torch.equal(obj['weights'][k], state[k]) for k in R.UNUSED)
    assert all(not torch.equal(obj['weights'][k], state[k]) for k in B.stat_names(state))
    assert int(obj['weights']['encoder._bn0.num_batches_tracked']) == int(state['encoder._bn0.num_batches_tracked']) + 2
    best = os.listdir(out / 'model')
    if best:
        sd = LinknetB4.from_checkpoint(str(out / 'model' / best[0]), gpu).state_dict()
        assert all(torch.equal(sd[k].cpu(), obj['weights'][k]) for k in obj['weights'])
    resume = str(out / 'checkpoints' / ck[0])
    history = train_image_seg.main(common + ['--epochs', '2', '--out-path', str(tmp_path / 'out2'), '--resume', resume, '--train-encoder'])
    assert [h[0] for h in history] == [1]
    ck2 = os.listdir(tmp_path / 'out2' / 'checkpoints')
    obj2 = torch.load(tmp_path / 'out2' / 'checkpoints' / ck2[0], map_location='cpu', weights_only=True)
    assert obj2['epoch'] == 1 and float(obj2['optimizer']['state'][0]['step']) == 4.0
    assert int(obj2['weights']['encoder._bn0.num_batches_tracked']) == int(state['encoder._bn0.num_batches_tracked']) + 4
    history = train_image_seg.main(common + ['--epochs', '2', '--out-path', str(tmp_path / 'out3'), '--resume', resume, '--freeze-encoder-statistics'])
    assert [h[0] for h in history] == [1]
    with pytest.raises(ValueError, match='train-encoder'):
        train_image_seg.main(common + ['--epochs', '2', '--out-path', str(tmp_path / 'out4'), '--model-path', resume, '--freeze-encoder'])
