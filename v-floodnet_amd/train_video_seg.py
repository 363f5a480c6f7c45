"""``train_video_seg.py`` of the reference on the HIP path: ``python -m vfloodnet_amd.train_video_seg --dataset DIR --resume CKPT``.

The reference's flags (train_video_seg.py:20-47) plus ``--size`` (the clip's edge, 400 in the reference: :95).  The epoch
loop (:150-181) runs ``train.train_model`` over a ``TrainClipLoader`` (the reference's ``DataLoader(Water_Image_Train_DS(...), shuffle=True, num_workers=2)``, :95-100) with ``train.AdamW`` and ``train.StepLR``;
resume, ``--new`` and the seed are handled as in :111-143; ``--log`` writes the checkpoints ``{epoch, model, optimizer, loss,
seed}`` as ``final.pth``, ``best.pth`` and ``epoch_XXX_loss_Y.pth`` (:157-179), which ``video_seg`` and the reference load.

One difference: the reference starts from torchvision's ImageNet weights (``load_imagenet_params=True``, :103), which are a
download.  Here the initial weights come from ``--resume`` (with ``--new`` to start the schedule afresh); without it the run
stops with an error instead of training from random weights.
"""
import argparse
import os
import time

import numpy as np
import torch

from . import train as T
from .model import AFB_URR
from .train_dataset import TrainClipLoader, Water_Image_Train_DS


def get_parser():
    parser = argparse.ArgumentParser(description='Train AFB-URR (MI355X-native)')
    parser.add_argument('--gpu', type=int, default=0, help='GPU card id.')
    parser.add_argument('--dataset', type=str, default=None, required=True, help='Dataset folder.')
    parser.add_argument('--seed', type=int, default=-1, help='Random seed.')
    parser.add_argument('--log', action='store_true', help='Save the training results.')
    parser.add_argument('--level', type=int, default=0, help='0: Water Image. 1: DAVIS. 2: Youtube-VOS.')
    parser.add_argument('--lr', type=float, default=1e-5, help='Learning rate, default 1e-5.')
    parser.add_argument('--lu', type=float, default=0.5, help='Regularization factor, default 0.5.')
    parser.add_argument('--resume', type=str, help='Path to the checkpoint (default: none)')
    parser.add_argument('--new', action='store_true', help='Train the model from the begining.')
    parser.add_argument('--scheduler-step', type=int, default=25, help='Scheduler step size. Default 25.')
    parser.add_argument('--total-epochs', type=int, default=100, help='Total running epochs. Default 100.')
    parser.add_argument('--budget', type=int, default=300000,
                        help='Max number of features that feature bank can store. Default: 300000')
    parser.add_argument('--obj-n', type=int, default=3, help='Max number of objects that will be trained at the same time.')
    parser.add_argument('--clip-n', type=int, default=6, help='Max frames that will be sampled as a batch.')
    parser.add_argument('--size', type=int, default=400, help='Edge of the training clips (reference: 400).')
    return parser


def gct():
    return time.strftime('%Y-%m-%d %H:%M:%S', time.localtime())


def main(argv=None):
    """-> {'loss': last epoch's mean loss, 'epochs': epochs run, 'model_path': checkpoint folder or None}."""
    args = get_parser().parse_args(argv)
    print(gct(), f'Args = {args}')
    if args.gpu >= 0 and torch.cuda.is_available():
        device = torch.device('cuda', args.gpu)
    else:
        raise ValueError('CUDA is required. --gpu must be >= 0.')
    if args.level != 0:
        raise ValueError(f'{args.level} is unknown.')
    if not args.resume:
        raise ValueError('--resume CHECKPOINT is required: the initial weights of the reference are a download '
                         '(load_imagenet_params=True); add --new to start the schedule from epoch 0')
    if not os.path.isfile(args.resume):
        print(gct(), f'No checkpoint found at {args.resume}')
        raise IOError(args.resume)

    model_path = None
    if args.log:
        log_dir = 'logs/{}'.format(time.strftime(f'level{args.level}' + '_%Y%m%d-%H%M%S'))
        model_path = os.path.join(log_dir, 'model')
        os.makedirs(os.path.join(log_dir, 'log'), exist_ok=True)
        os.makedirs(model_path, exist_ok=True)
        print(gct(), f'Create log dir: {log_dir}')

    dataset = Water_Image_Train_DS(args.dataset, output_size=args.size, clip_n=args.clip_n, max_obj_n=args.obj_n)
    print(gct(), f'Load level {args.level} dataset: {len(dataset)} training cases.')

    torch.cuda.set_device(device)
    model = AFB_URR(device, update_bank=False, load_imagenet_params=False).to(device)
    checkpoint = torch.load(args.resume, map_location='cpu')
    model.load_state_dict(checkpoint['model'], strict=False)
    model.train()                                      # (BatchNorm stays on its running statistics: train.py)
    optimizer = T.AdamW(model.named_parameters(), lr=args.lr)

    start_epoch, best_loss = 0, 100000000
    seed = checkpoint['seed']
    if not args.new:
        start_epoch = checkpoint['epoch'] + 1
        optimizer.load_state_dict(checkpoint['optimizer'])
        best_loss = checkpoint['loss']
        print(gct(), f'Loaded checkpoint {args.resume} (epoch: {start_epoch - 1}, best loss: {best_loss})')
    else:
        seed = int(time.time()) if args.seed < 0 else args.seed
        print(gct(), f'Loaded checkpoint {args.resume}. Train from the beginning.')
    print(gct(), 'Random seed:', seed)
    torch.manual_seed(seed)
    np.random.seed(seed % (1 << 32))

    loader = TrainClipLoader(dataset, device, shuffle=True, num_workers=2, seed=seed)
    loader.epoch = start_epoch                         # (a resumed run continues the seed's sequence of samples)
    scheduler = T.StepLR(optimizer, step_size=args.scheduler_step, gamma=0.5, last_epoch=start_epoch - 1)

    loss, epochs = float('nan'), 0
    for epoch in range(start_epoch, args.total_epochs):
        print('')
        print(gct(), f'Epoch: {epoch} lr: {scheduler.get_last_lr()[0]}')
        loss = T.train_model(model, loader, optimizer, lu=args.lu, budget=args.budget)
        epochs += 1
        print(gct(), f'loss {loss:.5f}')
        if args.log:
            ckpt = {'epoch': epoch, 'model': {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
                    'optimizer': optimizer.state_dict(), 'loss': loss, 'seed': seed}
            torch.save(ckpt, f'{model_path}/final.pth')
            if best_loss > loss:
                best_loss = loss
                torch.save(ckpt, f'{model_path}/epoch_{epoch:03d}_loss_{loss:.03f}.pth')
                torch.save(ckpt, f'{model_path}/best.pth')
                print('Best model updated.')
        scheduler.step()
    print(gct(), 'Training done.')
    return {'loss': loss, 'epochs': epochs, 'model_path': model_path}


if __name__ == '__main__':
    main()
