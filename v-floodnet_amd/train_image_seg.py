"""Fine-tuning the bootstrap LinkNet on a labelled set: the training half of ``train_image_seg.py`` on the GPU
(``linknet_train``).  ``freeze_encoder`` has four values: ``True`` trains decoder and head (include/vfn_image_train.h holds the
definition), ``'statistics'`` trains the encoder as well, on its running BatchNorm statistics and without drop-connect
(include/vfn_encoder_train.h), ``'train'`` trains it in train mode -- batch-statistics BatchNorm and drop-connect, the
reference's own ``model.train()`` (include/vfn_encoder_bn_train.h) -- and ``False`` is still refused: it is the reference's
spelling of ``'train'``, and three tests pin the refusal; making it an alias is a follow-up that edits them.

    TrainEpoch(model, device, optimizer, freeze_encoder=True).run(loader)   smp's TrainEpoch: one pass, the mean logs
    train_model(model, init_lr, num_epochs, out_path, train_loader, val_loader, encoder_name, device)   train_image_seg.py:112-203

    python -m vfloodnet_amd.train_image_seg --dataset-path D --encoder efficientnet-b4 --model-path F --freeze-encoder
    python -m vfloodnet_amd.train_image_seg --dataset-path D --encoder efficientnet-b4 --model-path F --freeze-encoder-statistics
    python -m vfloodnet_amd.train_image_seg --dataset-path D --encoder efficientnet-b4 --model-path F --train-encoder

Differences from the reference, on purpose:

* the best model is written as a state dict (``LinknetB4.from_checkpoint`` and ``val_image_seg`` load it), not as a pickled smp
  module: the package is no dependency;
* no matplotlib plots;
* no ImageNet download: ``--model-path`` / ``--resume`` supplies the starting weights (a pickled module, a state dict, or a
  resume checkpoint, whose optimizer state ``--resume`` restores as well);
* ``freeze_encoder=False`` raises ``NotImplementedError`` and names ``freeze_encoder='train'`` (``--train-encoder``), which is that
  mode; the drop-connect draws come from a host generator seeded by ``--seed`` and the epoch, not from torch's device stream.
Everything runs on the GPU; there is no CPU fallback.
"""
import os

import torch

from .linknet_train import (Adam, DecoderTrainer, ENCODER_MISSING, FullTrainer, ModelTrainer, UNUSED, freeze_encoder as _freeze,
                            freeze_encoder_statistics, train_mode)
from .val_image_seg import LOG_ROWS, ValidEpoch, load_checkpoint

ENCODER = 'efficientnet-b4'
DEFAULT_CHKPT_DIR = os.path.join('./', 'output', 'img_seg_checkpoint')
LR_SECOND_HALF = 1e-5
STATISTICS = 'statistics'
TRAIN = 'train'


def _check_mode(freeze_encoder):
    """True, 'statistics' or 'train'; False (the reference's spelling of 'train') is refused by a message that names 'train'."""
    if freeze_encoder is False or freeze_encoder is None or freeze_encoder == 0:
        raise NotImplementedError(ENCODER_MISSING)
    if freeze_encoder is not True and freeze_encoder not in (STATISTICS, TRAIN):
        raise ValueError(f"freeze_encoder is True, 'statistics', 'train' or False, got {freeze_encoder!r}")
    return freeze_encoder


def new_optimizer(model, freeze_encoder, init_lr):
    """The mode's ``Adam`` over the model's parameters (the model in that mode)."""
    mode = _check_mode(freeze_encoder)
    if mode is not True:
        return Adam((freeze_encoder_statistics if mode == STATISTICS else train_mode)(model).named_parameters(), lr=init_lr, skip=UNUSED)
    return Adam(_freeze(model).named_parameters(), lr=init_lr)


def load_optimizer_state(optimizer, sd, freeze_encoder):
    """``optimizer.load_state_dict(sd)`` for a resume checkpoint; one written for another set of parameters is refused by name
    ('statistics' and 'train' optimise the same 465 of 468 tensors and resume each other)."""
    n = sum(len(g['params']) for g in sd['param_groups'])
    if n != optimizer.n_group:
        mode = lambda k: {52: "freeze_encoder=True (--freeze-encoder)",
                          468: "freeze_encoder='statistics' (--freeze-encoder-statistics) or freeze_encoder='train' (--train-encoder)"}.get(
            k, 'another model')
        raise ValueError(f"the checkpoint's optimizer holds {n} parameters: it was written with {mode(n)}; this run trains {optimizer.n_group} "
                         f'with {mode(optimizer.n_group)}.  Resume in the mode the checkpoint was written in, or start from its weights alone')
    optimizer.load_state_dict(sd)


class TrainEpoch:
    """smp's ``TrainEpoch(model, loss=DiceLoss(), metrics=[IoU(threshold=0.5)], optimizer=optimizer, device=device)``
    (train_image_seg.py:144-151).  ``optimizer``: a ``linknet_train.Adam`` over the parameters that are trained, or None for a
    fresh one at ``init_lr``.  ``run(loader)`` takes ``(x, y)`` device batches, makes one optimisation step per batch and
    returns ``{'dice_loss': float, 'iou_score': float}``: the means over the batches (smp's ``AverageValueMeter``) of loss and
    score of the training-mode prediction each step started from.  The per-batch values stay on the device until the end of the
    epoch: one read-back.  ``log`` keeps it, f64 [batches, 2]."""

    def __init__(self, model, device, optimizer=None, freeze_encoder=True, init_lr=1e-4, verbose=True, seed=0):
        mode = _check_mode(freeze_encoder)
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('TrainEpoch runs on the GPU only (no CPU fallback)')
        self.model, self.device, self.verbose = model, device, verbose
        if mode == TRAIN:
            self.trainer = FullTrainer(model, init_lr=init_lr, optimizer=optimizer, seed=seed)
        else:
            self.trainer = (ModelTrainer if mode == STATISTICS else DecoderTrainer)(model, init_lr=init_lr, optimizer=optimizer)
        self.optimizer = self.trainer.optimizer
        self.log = None

    def reseed(self, epoch):
        """The head of an epoch: the drop-connect draws of ``'train'`` follow from (seed, epoch); the other modes draw nothing."""
        if isinstance(self.trainer, FullTrainer):
            self.trainer.reseed(epoch)

    def run(self, loader):
        blocks, t = [], 0
        with torch.cuda.device(self.device):
            for x, y in loader:
                if t % LOG_ROWS == 0:
                    blocks.append(torch.empty(LOG_ROWS, 2, dtype=torch.float64, device=self.device))
                logs = self.trainer.step(x, y)
                blocks[-1][t % LOG_ROWS, 0] = logs['dice_loss']
                blocks[-1][t % LOG_ROWS, 1] = logs['iou_score']
                t += 1
            if t == 0:
                raise ValueError('the loader produced no batch')
            self.log = torch.cat(blocks)[:t].cpu().numpy()           # the epoch's one read-back
        sums = [0.0, 0.0]
        for row in self.log:
            sums[0] += float(row[0])
            sums[1] += float(row[1])
        logs = {'dice_loss': sums[0] / t, 'iou_score': sums[1] / t}
        if self.verbose:
            print('train: dice_loss - {:.4}, iou_score - {:.4}'.format(logs['dice_loss'], logs['iou_score']))     # smp's log line
        return logs


def train_model(model, init_lr, num_epochs, out_path, train_loader, val_loader, encoder_name=ENCODER, device=None, freeze_encoder=True,
                optimizer=None, train_epoch=None, valid_epoch=None, start_epoch=0, seed=0):
    """``train_model`` of train_image_seg.py:112-203.  Per epoch: ``TrainEpoch``, then ``ValidEpoch``; the resume checkpoint
    ``checkpoints/epoch_###_score<score>.pth = {'epoch', 'weights', 'optimizer', 'loss': {}}`` (``DiceLoss`` has no state); when
    ``score > max_score`` the best model ``model/linknet_<encoder>_epoch_###_score<score>.pth`` (a state dict); at
    ``epoch == int(num_epochs / 2)`` the learning rate drops to 1e-5.  ``train_epoch`` / ``valid_epoch``: objects with
    ``run(loader)`` in place of the two epochs (tests).  ``seed``: of the drop-connect draws of ``freeze_encoder='train'``, which
    restart from (seed, epoch) at the head of every epoch, so a resumed run continues the sequence.  Returns the list of (epoch,
    train logs, valid logs, best or not)."""
    _check_mode(freeze_encoder)
    checkpoints_dir, models_dir = os.path.join(out_path, 'checkpoints'), os.path.join(out_path, 'model')
    os.makedirs(checkpoints_dir, exist_ok=True)
    os.makedirs(models_dir, exist_ok=True)
    if train_epoch is None:
        train_epoch = TrainEpoch(model, device, optimizer, freeze_encoder=freeze_encoder, init_lr=init_lr, seed=seed)
        optimizer = train_epoch.optimizer
    if valid_epoch is None:
        valid_epoch = ValidEpoch(model, device)
    max_score, history = 0, []
    for epoch in range(start_epoch, num_epochs):
        print('\nEpoch: {}'.format(epoch))
        if hasattr(train_epoch, 'reseed'):
            train_epoch.reseed(epoch)
        train_logs = train_epoch.run(train_loader)
        valid_logs = valid_epoch.run(val_loader)
        print('valid: dice_loss - {:.4}, iou_score - {:.4}'.format(valid_logs['dice_loss'], valid_logs['iou_score']))
        checkpoint = {'epoch': epoch, 'weights': {k: v.detach().clone() for k, v in model.state_dict().items()},
                      'optimizer': optimizer.state_dict(), 'loss': {}}
        score = float(valid_logs['iou_score'])
        torch.save(checkpoint, os.path.join(checkpoints_dir, 'epoch_' + str(epoch).zfill(3) + '_score' + str(score) + '.pth'))
        best = score > max_score
        if best:
            max_score = score
            torch.save(checkpoint['weights'],
                       os.path.join(models_dir, 'linknet_' + encoder_name + '_epoch_' + str(epoch).zfill(3) + '_score' + str(score) + '.pth'))
            print('New best model detected.')
        if epoch == int(num_epochs / 2):
            optimizer.lr = LR_SECOND_HALF
            print('Decrease decoder learning rate to 1e-5!')
        history.append((epoch, train_logs, valid_logs, best))
    return history


def get_args(argv=None):
    import argparse
    parser = argparse.ArgumentParser(description='Fine-tune the LinkNet on the MI355X (train_image_seg.py): decoder and head, or the whole '
                                                 'model with the encoder on its running BatchNorm statistics or in train mode.')
    parser.add_argument('--dataset-path', type=str, metavar='PATH', required=True,
                        help='Dataset root: train_imgs.txt, JPEGImages/<sub>/*.jpg, Annotations/<sub>/*.png.')
    parser.add_argument('--encoder', type=str, default=ENCODER, help='Encoder name; only efficientnet-b4 is built.')
    parser.add_argument('--input-shape', default=416, type=int, help='Input size of the model, a multiple of 32.')
    parser.add_argument('--batch-size', default=4, type=int, help='Batch size for mini-batch gradient descent.')
    parser.add_argument('--init-lr', default=1e-4, type=float, help='Initial learning rate; 1e-5 from half-way on.')
    parser.add_argument('--epochs', default=300, type=int, help='Number of epochs.')
    parser.add_argument('--out-path', default=DEFAULT_CHKPT_DIR, type=str, metavar='PATH', help='Output folder.')
    parser.add_argument('--model-path', '--resume', dest='model_path', type=str, metavar='PATH', required=True,
                        help='Starting weights: a pickled module, a state dict or a resume checkpoint (no ImageNet download).')
    mode = parser.add_mutually_exclusive_group()
    mode.add_argument('--freeze-encoder', action='store_true', help='Train decoder and head only.')
    mode.add_argument('--freeze-encoder-statistics', action='store_true',
                      help='Train the encoder as well, on its running BatchNorm statistics and without drop-connect.')
    mode.add_argument('--train-encoder', action='store_true',
                      help='Train the encoder as well, in train mode: batch-statistics BatchNorm and drop-connect (the reference).  One of '
                           'the three flags is required.')
    parser.add_argument('--seed', default=0, type=int, help='Seed of the shuffle, the augmentation draws and the drop-connect draws.')
    parser.add_argument('--num-workers', default=4, type=int, help='Loader processes for the host part of the decoding.')
    parser.add_argument('--gpu', default=0, type=int, help='GPU card id.')
    return parser.parse_args(argv)


def main(argv=None):
    from .image_dataset import ImageSampleLoader, WaterDataset_RGB
    args = get_args(argv)
    if args.encoder != ENCODER:
        raise ValueError(f'--encoder {args.encoder!r}: only {ENCODER} is built')
    if not args.freeze_encoder and not args.freeze_encoder_statistics and not args.train_encoder:
        raise NotImplementedError(ENCODER_MISSING.replace("freeze_encoder='statistics'", '--freeze-encoder-statistics')
                                  .replace("freeze_encoder='train'", '--train-encoder').replace('freeze_encoder=True', '--freeze-encoder'))
    freeze = TRAIN if args.train_encoder else STATISTICS if args.freeze_encoder_statistics else True
    if not torch.cuda.is_available() or args.gpu < 0:
        raise ValueError('CUDA is required. --gpu must be >= 0.')
    if args.input_shape < 32 or args.input_shape % 32:
        raise ValueError('--input-shape must be a multiple of 32 (the image is subsampled 5 times)')
    device = torch.device('cuda', args.gpu)
    # train_image_seg.py:56-80: both sets are train_offline samples of the one folder, the training set shuffled (the reference
    # fixes the training size at 416, its default --input-shape; here both sets take --input-shape)
    train_dataset = WaterDataset_RGB('train_offline', args.dataset_path, (args.input_shape, args.input_shape))
    val_dataset = WaterDataset_RGB('train_offline', args.dataset_path, (args.input_shape, args.input_shape))
    if len(train_dataset) == 0:
        raise ValueError(f'{args.dataset_path}: no labelled photograph found')
    train_loader = ImageSampleLoader(train_dataset, device, batch_size=args.batch_size, shuffle=True, num_workers=args.num_workers, seed=args.seed)
    val_loader = ImageSampleLoader(val_dataset, device, batch_size=1, shuffle=False, num_workers=args.num_workers, seed=args.seed + 1)
    model = load_checkpoint(args.model_path, device)
    optimizer = new_optimizer(model, freeze, args.init_lr)
    start_epoch = 0
    try:
        obj = torch.load(args.model_path, map_location='cpu', weights_only=True)
    except Exception:
        obj = None
    if isinstance(obj, dict) and 'optimizer' in obj and 'weights' in obj:      # a resume checkpoint of train_model
        load_optimizer_state(optimizer, obj['optimizer'], freeze)
        start_epoch = int(obj.get('epoch', -1)) + 1
    history = train_model(model, args.init_lr, args.epochs, args.out_path, train_loader, val_loader, args.encoder, device,
                          freeze_encoder=freeze, optimizer=optimizer, start_epoch=start_epoch, seed=args.seed)
    print('Done.')
    return history


if __name__ == '__main__':
    main()
